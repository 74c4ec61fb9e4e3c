"""GPU (MI355X): the calls that mirror the reference's own functions one to one -- the dense tree (imt_tree_*), the bare
permutation, the 128-bit split, the zero-hash chain and the subtree-root combiner -- at the edges of their kernels and
launch decisions, bit for bit against tests/mirror_corpus.py (pinned on the CPU by tests/test_mirror_corpus.py).

What varies: the number of items against the 256-thread block (one short, exact, one over, several blocks), which of
the two forms of a tree level runs (launch::tree_level: a quad of lanes per hash while n_parents * 4 <=
IMT_OPT_COOP_MAX_EVENTS, one thread per hash above), with the switch between two levels of ONE tree; the three
boundary formats on the way in and on the way out; host pointers and device pointers; both sibling layouts; the edge
values of the field in every position; and every refusal the header names, each with the output untouched or at least
the bytes around it.

What these tests cannot see: WHERE the switch between the two forms of a level falls.  Both forms must give the same
bytes, and that is what is asserted on both sides of the switch; a boundary moved by one (`<` for `<=`) changes no
output, and the C ABI has no counter of which kernel ran."""
import contextlib
import ctypes
import random

import numpy as np
import pytest

import mirror_corpus as mc
from mirror_corpus import FMTS, GUARD, R_OF, SENTINEL, check_guards, from_fmt, guarded, to_fmt
from oracle_lib import P, arr_ints, ints_to_arr

pytestmark = pytest.mark.gpu

FORMS = ("default", "thread", "quad", "switch64")
SIZES = (1, 2, 4, 64, 512, 1024)      # level 1 of 512 leaves is exactly one 256-thread block, of 1024 leaves two
BIG = 1 << 14                         # default context: level 1 (8192 parents) one thread per hash, 4096 and fewer a quad
BATCH = (0, 1, 255, 256, 257, 1000)   # items against the block: none, one, one short, exact, one over, ragged
NONCANONICAL = (P, (1 << 256) - 1)


def vp(x):
    return ctypes.c_void_p(int(x))


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got.reshape(-1, 32) != want.reshape(-1, 32)).any(axis=1))
    assert bad.size == 0, (what, "first elements that differ:", bad[:6, 0].tolist())


class Case:
    """one set of leaves, its model, and the model's levels in each boundary format (computed once)"""

    def __init__(self, leaves):
        self.m = mc.dense_model(leaves)
        self.n, self.depth = self.m.n, self.m.depth
        self._lv = {}

    def level(self, l, fmt):
        if (l, fmt) not in self._lv:
            self._lv[(l, fmt)] = to_fmt(self.m.levels[l], fmt)
        return self._lv[(l, fmt)]

    def leaf(self, i):
        return arr_ints(self.m.levels[0][i])[0]

    def proof(self, i, fmt):
        if not self.depth:
            return np.zeros((0, 32), np.uint8)
        return np.stack([self.level(l, fmt)[(i >> l) ^ 1] for l in range(self.depth)])

    def proofs(self, idx, fmt, item_major):
        """[n][depth][32] or [depth][n][32]"""
        if not len(idx):
            return np.zeros((0, self.depth, 32) if item_major else (self.depth, 0, 32), np.uint8)
        a = np.stack([self.proof(i, fmt) for i in idx])
        return a if item_major else np.ascontiguousarray(a.transpose(1, 0, 2))

    def helper(self, i, fmt):
        return ints_to_arr([h * R_OF[fmt] % P for h in self.m.helper(i)])

    def concatenated(self, fmt):
        return np.concatenate([self.level(l, fmt) for l in range(self.depth + 1)])


@pytest.fixture(scope="module")
def forms(imt, ctx):
    """the default context (a level of more than 4096 parents runs one thread per hash), thread per hash for every size
    (IMT_OPT_COOP_MAX_EVENTS = 0), quad per hash for every size (1 << 30), and 64: in a 64-leaf tree the level of 32
    parents runs k_tree_level and the levels of 16 and fewer the quad form"""
    made = {"thread": 0, "quad": 1 << 30, "switch64": 64}
    for k, v in list(made.items()):
        made[k] = imt.Context(0)
        made[k].set_option(imt._ffi.OPT_COOP_MAX_EVENTS, v)
    yield dict(default=ctx, **made)
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def cases(oracle):
    return {n: Case(ints_to_arr(mc.mixed_values(n, 0x4D490000 + n))) for n in SIZES}


@pytest.fixture(scope="module")
def big(oracle):
    return Case(ints_to_arr(mc.mixed_values(BIG, 0x4D49B16)))


@contextlib.contextmanager
def dense(imt, c, leaves, flags=0):
    """imt_tree_new over host bytes `leaves` (or a device address, with n, as a pair); freed on exit"""
    h = ctypes.c_void_p()
    if isinstance(leaves, tuple):
        rc = imt.lib.imt_tree_new(c.h, vp(leaves[0]), leaves[1], flags, ctypes.byref(h))
    else:
        a = np.ascontiguousarray(leaves, dtype=np.uint8)
        rc = imt.lib.imt_tree_new(c.h, ptr(a), a.shape[0], flags, ctypes.byref(h))
    assert rc == 0 and h.value, (rc, imt.lib.imt_last_error(c.h))
    try:
        yield h
    finally:
        imt.lib.imt_tree_free(h)


def get_level(imt, t, l, fmt):
    n = ctypes.c_size_t(12345)
    assert imt.lib.imt_tree_get_level(t, l, None, ctypes.byref(n), fmt) == 0           # the length alone
    g = guarded((n.value, 32))
    n2 = ctypes.c_size_t(54321)
    assert imt.lib.imt_tree_get_level(t, l, vp(g.ptr), ctypes.byref(n2), fmt) == 0
    assert n2.value == n.value
    return check_guards(g)


def check_tree(imt, t, case, what, read_fmts=FMTS):
    assert imt.lib.imt_tree_num_levels(t) == case.depth + 1
    for fmt in read_fmts:
        for l in range(case.depth + 1):
            got = get_level(imt, t, l, fmt)
            assert got.shape == (case.n >> l, 32), (what, l)
            same(got, case.level(l, fmt), (what, "read as", fmt, "level", l))
        g = guarded(32)
        assert imt.lib.imt_tree_get_root(t, vp(g.ptr), fmt) == 0
        assert (check_guards(g) == case.level(case.depth, fmt)[0]).all(), (what, "root read as", fmt)
    n = ctypes.c_size_t(777)
    g = guarded(32)
    assert imt.lib.imt_tree_get_level(t, case.depth + 1, vp(g.ptr), ctypes.byref(n), 0) == imt._ffi.ERR["RANGE"]
    assert g.untouched() and n.value == 777


def verifies(imt, c, oracle, case, idx, level_major_canonical):
    """verify_proof (src/utils.rs:87-107) accepts every returned proof with its own leaf and index against the tree's
    root, on the GPU and by the oracle's path walk"""
    idx = [int(i) for i in idx]
    if not idx:
        return
    for k, i in enumerate(idx):
        assert oracle.path_root(case.leaf(i), i, level_major_canonical[:, k]) == case.m.root, i
    if case.depth:
        ok = c.verify_proof_batch(case.m.levels[0][idx], idx, case.m.levels[-1][0], level_major_canonical, case.depth)
        assert ok.all()


# ======================================================================================================= dense tree
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", FORMS)
def test_dense_tree_levels_do_not_depend_on_the_input_format(imt, forms, cases, form, n):
    """built from each format, every level, its length, num_levels and the root read back in each format"""
    c, case = forms[form], cases[n]
    for fmt_in in FMTS:
        with dense(imt, c, case.level(0, fmt_in), fmt_in) as t:
            check_tree(imt, t, case, (form, n, "built from", fmt_in))


def test_dense_tree_where_the_default_switch_falls(imt, ctx, big):
    """2^14 leaves in the default context: 8192 parents one thread per hash, 4096 parents and fewer a quad per hash"""
    for fmt_in in FMTS:
        with dense(imt, ctx, big.level(0, fmt_in), fmt_in) as t:
            check_tree(imt, t, big, ("2^14 built from", fmt_in), read_fmts=(fmt_in, (fmt_in + 1) % 3))


@pytest.mark.parametrize("form", FORMS)
def test_dense_tree_of_equal_leaves_is_the_zero_chain(imt, forms, form):
    z = mc.zero_chain(10)
    with dense(imt, forms[form], ints_to_arr([z[0]] * 1024)) as t:
        for l in range(11):
            assert arr_ints(get_level(imt, t, l, 0)) == [z[l]] * (1024 >> l), l


@pytest.mark.parametrize("form", FORMS)
def test_tree_build_writes_the_levels_bottom_up(imt, forms, cases, form):
    """imt_tree_build: levels [2n - 1][32] and root, either or both NULL, n = 1 included, in every format"""
    c = forms[form]
    for n in (1, 2, 64, 1024):
        case = cases[n]
        for fmt in FMTS:
            leaves = case.level(0, fmt)
            want_lv, want_root = case.concatenated(fmt), case.level(case.depth, fmt)[0]
            assert want_lv.shape == (2 * n - 1, 32)
            for with_levels, with_root in ((True, True), (False, True), (True, False), (False, False)):
                lv, rt = guarded((2 * n - 1, 32)), guarded(32)
                rc = imt.lib.imt_tree_build(c.h, ptr(leaves), n, vp(lv.ptr) if with_levels else None,
                                            vp(rt.ptr) if with_root else None, fmt)
                assert rc == 0, (n, fmt, with_levels, with_root, imt.lib.imt_last_error(c.h))
                if with_levels:
                    same(check_guards(lv), want_lv, (form, n, fmt, "levels"))
                else:
                    assert lv.untouched()
                if with_root:
                    assert (check_guards(rt) == want_root).all(), (form, n, fmt, "root")
                else:
                    assert rt.untouched()
    bad = cases[64].level(0, 0).copy()
    bad[17] = ints_to_arr([P])[0]
    lv, rt = guarded((127, 32)), guarded(32)
    assert imt.lib.imt_tree_build(c.h, ptr(bad), 64, vp(lv.ptr), vp(rt.ptr), 0) == imt._ffi.ERR["NONCANONICAL"]
    assert lv.untouched() and rt.untouched()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", FORMS)
def test_get_proof_and_helper_in_every_format(imt, forms, cases, oracle, form, n):
    """every index of a small tree, the first, the last and both sides of the middle of a larger one; the helper is 1 for
    a left child and 0 for a right one (src/utils.rs:79), scaled like any element of the format"""
    c, case = forms[form], cases[n]
    d = case.depth
    idx = list(range(n)) if n <= 64 else [0, 1, n // 2 - 1, n // 2, n - 1]
    with dense(imt, c, case.level(0, 0)) as t:
        got0 = []
        for fmt in FMTS:
            for i in idx:
                pr, hp = guarded((d, 32)), guarded((d, 32))
                assert imt.lib.imt_tree_get_proof(t, i, vp(pr.ptr), vp(hp.ptr), fmt) == 0
                if d:
                    same(check_guards(pr), case.proof(i, fmt), (form, n, fmt, i, "proof"))
                    same(check_guards(hp), case.helper(i, fmt), (form, n, fmt, i, "helper"))
                else:
                    assert pr.untouched() and hp.untouched()
                if fmt == 0:
                    got0.append(pr.body.copy())
            pr = guarded((d, 32))                                   # helper = NULL: the siblings alone
            assert imt.lib.imt_tree_get_proof(t, idx[-1], vp(pr.ptr), None, fmt) == 0
            same(check_guards(pr), case.proof(idx[-1], fmt), (form, n, fmt, "helper NULL"))
            for beyond in (n, n + 1, 1 << 40):
                pr, hp = guarded((d, 32)), guarded((d, 32))
                assert imt.lib.imt_tree_get_proof(t, beyond, vp(pr.ptr), vp(hp.ptr), fmt) == imt._ffi.ERR["RANGE"]
                assert pr.untouched() and hp.untouched()
        verifies(imt, c, oracle, case, idx, np.stack(got0, axis=1) if d else np.zeros((0, len(idx), 32), np.uint8))


@pytest.fixture(scope="module")
def big_tree(imt, ctx, big):
    with dense(imt, ctx, big.level(0, 0)) as t:
        yield t


def proof_batch(imt, t, idx, depth, fmt, item_major):
    idx = np.ascontiguousarray(idx, dtype=np.uint64)
    n = idx.size
    g = guarded((n, depth, 32) if item_major else (depth, n, 32))
    hold = idx if n else np.zeros(1, np.uint64)
    rc = imt.lib.imt_tree_get_proof_batch(t, ptr(hold), n, vp(g.ptr), fmt | (imt._ffi.SIB_ITEM_MAJOR if item_major else 0))
    return rc, g


@pytest.mark.parametrize("n", [0, 1, 18, 19, 257])
def test_get_proof_batch_ragged_against_the_block(imt, ctx, oracle, big, big_tree, n):
    """depth 14: n * depth = 0 / 14 / 252 / 266 / 3598 threads against 256-thread blocks, items fastest"""
    rng = random.Random(1400 + n)
    idx = ([0, BIG - 1, BIG // 2, BIG // 2 - 1] + [rng.randrange(BIG) for _ in range(n)])[:n]
    if n >= 18:
        idx[7] = idx[3]                                             # a repeated index
    for fmt in FMTS:
        for item_major in (False, True):
            rc, g = proof_batch(imt, big_tree, idx, big.depth, fmt, item_major)
            assert rc == 0
            same(check_guards(g), big.proofs(idx, fmt, item_major), (n, fmt, item_major))
            if fmt == 0 and not item_major:
                verifies(imt, ctx, oracle, big, idx, g.body)


@pytest.mark.parametrize("form", ("default", "switch64"))
def test_get_proof_batch_every_index_both_layouts(imt, forms, cases, oracle, form):
    c, case = forms[form], cases[64]
    idx = list(range(64)) + [63, 0, 7, 7, 7]
    with dense(imt, c, case.level(0, 1), 1) as t:
        for fmt in FMTS:
            for item_major in (False, True):
                rc, g = proof_batch(imt, t, idx, 6, fmt, item_major)
                assert rc == 0
                same(check_guards(g), case.proofs(idx, fmt, item_major), (form, fmt, item_major))
                if fmt == 0 and not item_major:
                    verifies(imt, c, oracle, case, idx, g.body)
                for beyond in (64, 65, 1 << 63):                    # host pointers: checked before anything is enqueued
                    bad = list(idx)
                    bad[30] = beyond
                    rc, g = proof_batch(imt, t, bad, 6, fmt, item_major)
                    assert rc == imt._ffi.ERR["RANGE"] and g.untouched(), (fmt, item_major, beyond)
        rc, g = proof_batch(imt, t, [], 6, 0, False)
        assert rc == 0 and g.untouched()


@pytest.mark.parametrize("form", ("default", "thread", "quad"))
def test_dense_tree_refuses_a_leaf_that_is_not_reduced(imt, forms, cases, form):
    """p and 2^256 - 1 as the bytes of the first leaf, the last, and leaf 300 of 1024, in each format: IMT_ERR_NONCANONICAL,
    no handle, and the context goes on working"""
    c, case = forms[form], cases[1024]
    for fmt in FMTS:
        for pos in (0, 1023, 300):
            for v in NONCANONICAL:
                leaves = case.level(0, fmt).copy()
                leaves[pos] = ints_to_arr([v])[0]
                h = ctypes.c_void_p(0xdead)
                rc = imt.lib.imt_tree_new(c.h, ptr(leaves), 1024, fmt, ctypes.byref(h))
                assert rc == imt._ffi.ERR["NONCANONICAL"] and not h.value, (form, fmt, pos, v)
        with dense(imt, c, case.level(0, fmt), fmt) as t:
            g = guarded(32)
            assert imt.lib.imt_tree_get_root(t, vp(g.ptr), 0) == 0
            assert arr_ints(check_guards(g)) == [case.m.root]


@pytest.fixture(scope="module")
def on_torch_stream(imt):
    """(torch, a context bound to torch's current stream); torch's own start-up happens here, once"""
    import torch
    torch.zeros(1, device="cuda").cpu()
    c2 = imt.Context(0)
    c2.set_stream(torch.cuda.current_stream().cuda_stream)
    yield torch, c2
    c2.close()


@pytest.mark.parametrize("which,fmt", [(64, 0), (1024, 1), (1024, 2), (BIG, 1)])
def test_dense_tree_through_device_pointers(imt, on_torch_stream, cases, big, which, fmt):
    """IMT_DEVICE_PTRS on a context bound to torch's stream: leaves from a torch tensor, levels, root and proofs into
    torch tensors with guard bytes around them and once into imt_host_alloc memory; equal to the model after sync.
    An index beyond the leaves, which the host cannot see here, reads the empty-subtree hashes (include/imt.h)."""
    torch, c2 = on_torch_stream
    F = imt._ffi
    dev = torch.device("cuda", 0)

    def d_guarded(nbytes):
        return torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)

    def d_body(raw, shape):
        host = raw.cpu().numpy()
        nbytes = host.size - 2 * GUARD
        assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + nbytes:] == SENTINEL).all(), "wrote outside the buffer"
        return host[GUARD:GUARD + nbytes].reshape(shape)

    z = mc.zero_chain(14)
    case = big if which == BIG else cases[which]
    n, d = case.n, case.depth
    leaves = torch.from_numpy(case.level(0, fmt)).to(dev)
    with dense(imt, c2, (leaves.data_ptr(), n), F.DEVICE_PTRS | fmt) as t:
        lv = [d_guarded((n >> l) * 32) for l in range(d + 1)]
        for l in range(d + 1):
            assert imt.lib.imt_tree_get_level(t, l, vp(lv[l].data_ptr() + GUARD), None, F.DEVICE_PTRS | fmt) == 0
        rt = d_guarded(32)
        assert imt.lib.imt_tree_get_root(t, vp(rt.data_ptr() + GUARD), F.DEVICE_PTRS | fmt) == 0
        idx = [0, n - 1, n // 2, n // 2 - 1, 5, 5] + list(range(0, n, max(1, n // 13)))
        d_idx = torch.from_numpy(np.array(idx, dtype=np.int64)).to(dev)
        out = {}
        for item_major in (False, True):
            out[item_major] = d_guarded(len(idx) * d * 32)
            flags = F.DEVICE_PTRS | fmt | (F.SIB_ITEM_MAJOR if item_major else 0)
            assert imt.lib.imt_tree_get_proof_batch(t, vp(d_idx.data_ptr()), len(idx), vp(out[item_major].data_ptr() + GUARD),
                                                    flags) == 0
        pinned = guarded((d, len(idx), 32), alloc=c2.host_alloc)
        pin_root = guarded(32, alloc=c2.host_alloc)
        assert imt.lib.imt_tree_get_proof_batch(t, vp(d_idx.data_ptr()), len(idx), vp(pinned.ptr), F.DEVICE_PTRS | fmt) == 0
        assert imt.lib.imt_tree_get_root(t, vp(pin_root.ptr), F.DEVICE_PTRS | fmt) == 0
        beyond = [n, n + 1, 2 * n + 3, (1 << 64) - 1]
        d_beyond = torch.from_numpy(np.array(beyond, dtype=np.uint64).view(np.int64)).to(dev)
        empty = d_guarded(len(beyond) * d * 32)
        assert imt.lib.imt_tree_get_proof_batch(t, vp(d_beyond.data_ptr()), len(beyond), vp(empty.data_ptr() + GUARD),
                                                F.DEVICE_PTRS | fmt) == 0
        # a one-element proof through imt_tree_get_proof is a host-pointer call
        assert imt.lib.imt_tree_get_proof(t, 0, vp(rt.data_ptr() + GUARD), None, F.DEVICE_PTRS) == F.ERR["ARG"]
        c2.sync()
        torch.cuda.synchronize()
        for l in range(d + 1):
            same(d_body(lv[l], (n >> l, 32)), case.level(l, fmt), (n, fmt, "device level", l))
        assert (d_body(rt, (32,)) == case.level(d, fmt)[0]).all()
        same(d_body(out[False], (d, len(idx), 32)), case.proofs(idx, fmt, False), (n, fmt, "device proofs"))
        same(d_body(out[True], (len(idx), d, 32)), case.proofs(idx, fmt, True), (n, fmt, "device proofs item-major"))
        same(check_guards(pinned), case.proofs(idx, fmt, False), (n, fmt, "pinned proofs"))
        assert (check_guards(pin_root) == case.level(d, fmt)[0]).all()
        want_empty = to_fmt(ints_to_arr(z[:d]), fmt)
        got_empty = d_body(empty, (d, len(beyond), 32))
        for k in range(len(beyond)):
            same(got_empty[:, k], want_empty, (n, fmt, "index beyond the leaves", beyond[k]))
        for g in (pinned, pin_root):
            c2.host_free(g.raw)
    # imt_tree_build with device pointers returns after its own sync
    if n <= 1024:
        lv, rt = d_guarded((2 * n - 1) * 32), d_guarded(32)
        assert imt.lib.imt_tree_build(c2.h, vp(leaves.data_ptr()), n, vp(lv.data_ptr() + GUARD), vp(rt.data_ptr() + GUARD),
                                      F.DEVICE_PTRS | fmt) == 0
        same(d_body(lv, (2 * n - 1, 32)), case.concatenated(fmt), (n, fmt, "device build"))
        assert (d_body(rt, (32,)) == case.level(d, fmt)[0]).all()
    # imt_tree_new is synchronous in this mode too: a leaf >= p is refused at the call
    bad = case.level(0, fmt).copy()
    bad[n // 3] = ints_to_arr([P])[0]
    d_bad = torch.from_numpy(bad).to(dev)
    h = ctypes.c_void_p(0xdead)
    assert imt.lib.imt_tree_new(c2.h, vp(d_bad.data_ptr()), n, F.DEVICE_PTRS | fmt, ctypes.byref(h)) == F.ERR["NONCANONICAL"]
    assert not h.value
    assert imt.lib.imt_ctx_sync(c2.h) == 0                      # and the error is not reported a second time


# ======================================================================================================= permutation
@pytest.fixture(scope="module")
def perm_pool(oracle):
    """1000 states, the special ones last so that every batch size ends in them: (0,0,0), (p-1,p-1,p-1) and each edge
    value in each lane; inputs and the oracle's outputs in each format"""
    rng = random.Random(0x9E44)
    special = [[0, 0, 0], [P - 1, P - 1, P - 1]]
    for e in mc.edge_values():
        for lane in range(3):
            s = [rng.randrange(P) for _ in range(3)]
            s[lane] = e
            special.append(s)
    states = [[rng.randrange(P) for _ in range(3)] for _ in range(1000 - len(special))] + special
    want = [oracle.permute(s) for s in states]
    assert all(x < P for w in want for x in w)
    a = ints_to_arr([x for s in states for x in s]).reshape(1000, 3, 32)
    b = ints_to_arr([x for w in want for x in w]).reshape(1000, 3, 32)
    return {fmt: (to_fmt(a, fmt), to_fmt(b, fmt)) for fmt in FMTS}


@pytest.mark.parametrize("n", BATCH)
def test_permute_batch_sizes_formats_and_refusals(imt, ctx, perm_pool, n):
    """imt_permute_batch, the test hook of the round schedule: one thread per state"""
    for fmt in FMTS:
        a, want = (np.ascontiguousarray(x[1000 - n:]) for x in perm_pool[fmt])
        g = guarded((n, 3, 32))
        assert imt.lib.imt_permute_batch(ctx.h, ptr(a) if n else None, vp(g.ptr), n, fmt) == 0
        same(check_guards(g) if n else g.body, want, ("permute", n, fmt))
        if fmt == 0:
            assert all(x < P for x in arr_ints(g.body))             # canonical bytes out, not merely congruent ones
        if not n:
            assert g.untouched()
            continue
        for lane in range(3):
            for v in NONCANONICAL:
                bad = a.copy()
                bad[n - 1, lane] = ints_to_arr([v])[0]
                g = guarded((n, 3, 32))
                assert imt.lib.imt_permute_batch(ctx.h, ptr(bad), vp(g.ptr), n, fmt) == imt._ffi.ERR["NONCANONICAL"], (n, fmt, lane)
                check_guards(g)
        g = guarded((n, 3, 32))                                     # and the context goes on working
        assert imt.lib.imt_permute_batch(ctx.h, ptr(a), vp(g.ptr), n, fmt) == 0
        same(check_guards(g), want, ("permute after a refusal", n, fmt))


def test_permute_batch_through_device_pointers(imt, on_torch_stream, perm_pool):
    """the result is the host mode's; a state that is not reduced is reported by the next imt_ctx_sync, once"""
    torch, c2 = on_torch_stream
    F = imt._ffi
    dev = torch.device("cuda", 0)
    for fmt in FMTS:
        for n in (257, 1000):
            a, want = (np.ascontiguousarray(x[1000 - n:]) for x in perm_pool[fmt])
            d_in = torch.from_numpy(a).to(dev)
            raw = torch.full((GUARD + n * 96 + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
            assert imt.lib.imt_permute_batch(c2.h, vp(d_in.data_ptr()), vp(raw.data_ptr() + GUARD), n, F.DEVICE_PTRS | fmt) == 0
            assert imt.lib.imt_ctx_sync(c2.h) == 0
            host = raw.cpu().numpy()
            assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n * 96:] == SENTINEL).all()
            same(host[GUARD:GUARD + n * 96].reshape(n, 3, 32), want, ("device permute", n, fmt))
        bad = a.copy()
        bad[500, 1] = ints_to_arr([P])[0]
        d_bad = torch.from_numpy(bad).to(dev)
        assert imt.lib.imt_permute_batch(c2.h, vp(d_bad.data_ptr()), vp(raw.data_ptr() + GUARD), 1000, F.DEVICE_PTRS | fmt) == 0
        assert imt.lib.imt_ctx_sync(c2.h) == F.ERR["NONCANONICAL"]
        assert imt.lib.imt_ctx_sync(c2.h) == 0


# ======================================================================================================= 128-bit split
@pytest.fixture(scope="module")
def split_pool():
    rng = random.Random(0x5B17)
    vals = [rng.randrange(P) for _ in range(700)]
    vals += [rng.randrange(1 << 128) for _ in range(100)]                          # q = 0
    vals += [rng.randrange(P >> 128) << 128 for _ in range(100)]                   # r = 0
    vals += [(P >> 128) << 128, ((P >> 128) << 128) - 1]                           # the largest q, and r all ones under it
    vals += [rng.randrange(P) for _ in range(1000 - len(vals) - len(mc.edge_values()))] + mc.edge_values()
    assert len(vals) == 1000 and all(0 <= v < P for v in vals)
    return vals


@pytest.mark.parametrize("n", BATCH)
def test_split128_sizes_formats_and_refusals(imt, ctx, split_pool, n):
    """q = v >> 128, r = v mod 2^128 (src/indexed_merkle_tree.rs:145-178), each an element of the call's format"""
    vals = split_pool[1000 - n:]
    for fmt in FMTS:
        a = to_fmt(ints_to_arr(vals), fmt) if n else np.zeros((0, 32), np.uint8)
        q, r = guarded((n, 32)), guarded((n, 32))
        assert imt.lib.imt_split128_batch(ctx.h, ptr(a) if n else None, vp(q.ptr), vp(r.ptr), n, fmt) == 0
        if not n:
            assert q.untouched() and r.untouched()
            continue
        gq, gr = arr_ints(from_fmt(check_guards(q), fmt)), arr_ints(from_fmt(check_guards(r), fmt))
        assert gq == [v >> 128 for v in vals], fmt
        assert gr == [v & mc.M128 for v in vals], fmt
        assert all((x << 128) + y == v for x, y, v in zip(gq, gr, vals))
        same(q.body, to_fmt(ints_to_arr([v >> 128 for v in vals]), fmt), ("q bytes", n, fmt))     # reduced bytes, not congruent ones
        same(r.body, to_fmt(ints_to_arr([v & mc.M128 for v in vals]), fmt), ("r bytes", n, fmt))
        for v in NONCANONICAL:
            for pos in {0, n - 1}:
                bad = a.copy()
                bad[pos] = ints_to_arr([v])[0]
                q, r = guarded((n, 32)), guarded((n, 32))
                assert imt.lib.imt_split128_batch(ctx.h, ptr(bad), vp(q.ptr), vp(r.ptr), n, fmt) == imt._ffi.ERR["NONCANONICAL"]
                check_guards(q), check_guards(r)


# ======================================================================================================= combiner
@pytest.fixture(scope="module")
def sub_roots():
    return {n: mc.mixed_values(n, 0xC0B0000 + n) for n in (1, 2, 8, 64, 1024, 16384)}


def combine(imt, c, roots_arr, n_roots, sub_height, depth, fmt):
    g = guarded(32)
    rc = imt.lib.imt_combine_subtree_roots(c.h, ptr(roots_arr), n_roots, sub_height, depth, vp(g.ptr), fmt)
    return rc, g


def shapes_of(k):
    return sorted({(0, k), (0, 64), (3, k + 3), (3, 32), (64 - k, 64)})


@pytest.mark.parametrize("n_roots", [1, 2, 8, 64, 1024])
@pytest.mark.parametrize("form", ("default", "thread", "quad"))
def test_combine_subtree_roots_shapes_and_formats(imt, forms, sub_roots, form, n_roots):
    """no level at all (one root: the extension alone), no extension (sub_height + k = depth), sub_height 0, depth 64"""
    c, roots = forms[form], sub_roots[n_roots]
    k = n_roots.bit_length() - 1
    for fmt in FMTS:
        a = to_fmt(ints_to_arr(roots), fmt)
        for sub_height, depth in shapes_of(k):
            rc, g = combine(imt, c, a, n_roots, sub_height, depth, fmt)
            assert rc == 0, (form, n_roots, sub_height, depth, fmt)
            want = mc.combined_root(roots, sub_height, depth) * R_OF[fmt] % P
            assert arr_ints(check_guards(g)) == [want], (form, n_roots, sub_height, depth, fmt)


def test_combine_subtree_roots_where_the_default_switch_falls(imt, ctx, sub_roots):
    """16384 roots in the default context: the first level of 8192 parents runs one thread per hash"""
    roots = sub_roots[16384]
    for fmt in FMTS:
        a = to_fmt(ints_to_arr(roots), fmt)
        for sub_height, depth in shapes_of(14):
            rc, g = combine(imt, ctx, a, 16384, sub_height, depth, fmt)
            assert rc == 0
            assert arr_ints(check_guards(g)) == [mc.combined_root(roots, sub_height, depth) * R_OF[fmt] % P], (sub_height, depth, fmt)


def test_combine_subtree_roots_refusals(imt, ctx, sub_roots):
    E = imt._ffi.ERR
    a = ints_to_arr(sub_roots[8])
    for n_roots in (0, 3, 6):
        rc, g = combine(imt, ctx, a, n_roots, 0, 32, 0)
        assert rc == E["ARG"] and g.untouched(), n_roots
    for n_roots, sub_height, depth in ((8, 0, 2), (8, 3, 5), (8, 62, 64), (1, 1, 0), (2, 64, 64), (1, 0, 65), (8, 3, 65)):
        rc, g = combine(imt, ctx, a, n_roots, sub_height, depth, 0)
        assert rc == E["RANGE"] and g.untouched(), (n_roots, sub_height, depth)
    for v in NONCANONICAL:
        bad = a.copy()
        bad[7] = ints_to_arr([v])[0]
        rc, g = combine(imt, ctx, bad, 8, 3, 32, 0)
        assert rc == E["NONCANONICAL"]
        check_guards(g)
    rc, g = combine(imt, ctx, a, 8, 3, 6, 0)                         # and the context goes on working
    assert rc == 0 and arr_ints(check_guards(g)) == [mc.combined_root(sub_roots[8], 3, 6)]


# ======================================================================================================= zero hashes
def zero_hashes(imt, c, depth, fmt):
    g = guarded((depth + 1, 32))
    return imt.lib.imt_zero_hashes(c.h, depth, vp(g.ptr), fmt), g


def test_zero_hashes_level_by_level_to_the_maximum_depth(imt, ctx):
    """Z[0] = H(0,0,0), Z[l+1] = H(Z[l], Z[l]) up to IMT_MAX_DEPTH = 64, from a context that has done other work and
    from one created just now (k_zero_chain runs at creation)"""
    z = mc.zero_chain(64)
    fresh = imt.Context(0)
    for c in (ctx, fresh):
        for depth in (0, 1, 32, 64):
            for fmt in FMTS:
                rc, g = zero_hashes(imt, c, depth, fmt)
                assert rc == 0
                same(check_guards(g), to_fmt(ints_to_arr(z[:depth + 1]), fmt), ("zero hashes", depth, fmt))
        rc, g = zero_hashes(imt, c, 65, 0)
        assert rc == imt._ffi.ERR["RANGE"] and g.untouched()
    fresh.close()


# ======================================================================================================= interleaving
def test_a_refused_call_a_tree_without_error_word_and_a_good_call(imt, forms, cases, oracle):
    """the quad form of a tree level is launched without the error word; next to calls that use it, each behaves as alone"""
    c, case = forms["switch64"], cases[64]
    bad = ints_to_arr([1, P]).reshape(1, 2, 32)
    for _ in range(2):
        with pytest.raises(imt.ImtError) as ei:
            c.hash2(bad)
        assert ei.value.code == imt._ffi.ERR["NONCANONICAL"]
        t = imt.IndexedMerkleTree.new(c, case.level(0, 0))
        assert t.get_root() == case.m.root
        for l in range(7):
            assert (t.get_level(l) == case.level(l, 0)).all()
        good = ints_to_arr([1, 2, P - 1, P - 2]).reshape(2, 2, 32)
        assert arr_ints(c.hash2(good)) == [oracle.hash([1, 2]), oracle.hash([P - 1, P - 2])]
        t.close()
