"""GPU (MI355X): the inline-assembly Montgomery forms, the helpers they feed and both permutation schedules, through the
test-only harness tests/native/fe_forms.hip, against tests/fe_model.py bit for bit as integers (not mod p) on each
form's operand corpus (tests/fe_corpus.py), and the permutations from non-canonical entries against the oracle and the
host build of the same schedule.  FE_FORMS_CSRC builds the harness against another copy of csrc/ (into that
directory), so that a changed form can be tried against these tests."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import fe_corpus as fc
import fe_model as fm
from fe_model import NL, P, W
from test_fe_forms import FORM_NAMES, check_exit, entry_states, host_permute

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.environ.get("FE_FORMS_CSRC") or os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def fe():
    """the harness, (re)built when it is missing or older than a source or a header it includes"""
    src = os.path.join(ROOT, "tests", "native", "fe_forms.hip")
    so = os.path.join(CSRC if os.environ.get("FE_FORMS_CSRC") else os.path.join(ROOT, "tests", "native"),
                      "libfe_forms.so")
    deps = [src] + [os.path.join(CSRC, f) for f in ("imt_params.cpp", "imt_params.hpp", "imt_fr_host.hpp",
                                                    "imt_device.hpp", "imt_consts.hpp", "imt_mont_asm.hpp",
                                                    "imt_trace_device.hpp", "imt_coop_device.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                            "-I", CSRC, "-o", so, src, os.path.join(CSRC, "imt_params.cpp")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    lib = ctypes.CDLL(so)
    lib.fe_form.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint,
                            ctypes.c_void_p, ctypes.c_uint]
    lib.fe_helper.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint,
                              ctypes.c_uint]
    lib.fe_permute.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    assert lib.fe_init() == 0
    return lib


@pytest.fixture(scope="module")
def tables(emul):
    buf = np.zeros(emul.emul_consts_size() // 4, np.uint32)
    emul.emul_consts_raw(_p(buf))
    tbuf = np.zeros(emul.emul_trace_consts_size() // 4, np.uint32)
    emul.emul_trace_consts_raw(_p(tbuf))
    return fc.parse(buf, fc.PC_LAYOUT), fc.parse(tbuf, fc.TC_LAYOUT)


def device_form(fe, name, X):
    """run one form's kernel on corpus rows: the lane slots per row, the uniform slots per block of fc.BLOCK rows"""
    doms = fc.DOMAINS[name]
    cs = [s for s, d in enumerate(doms) if d == fc.CONST]
    ls = [s for s, d in enumerate(doms) if d != fc.CONST]
    n = X.shape[0]
    lanes = np.ascontiguousarray(X[:, ls].astype(np.uint32))
    uni = np.ascontiguousarray(X[::fc.BLOCK][:, cs].astype(np.uint32)) if cs else np.zeros(1, np.uint32)
    if cs:   # the corpus keeps its constants uniform per block: the harness can only read one set per block
        blk = X[:, cs].reshape(-1, len(cs) * NL)
        assert (blk == np.repeat(blk[::fc.BLOCK], fc.BLOCK, axis=0)[:n]).all()
    out = np.zeros((n, NL), np.uint32)
    assert fe.fe_form(name.encode(), _p(lanes), len(ls), _p(uni), len(cs), _p(out), n) == 0
    return out


@pytest.mark.parametrize("name", FORM_NAMES)
def test_form_matches_model(fe, tables, name):
    X = fc.corpus(name, *tables)
    assert X.shape[0] % fc.BLOCK != 0          # ragged: the last wave is partial
    want = fc.model(name, X)[0].astype(np.uint32)
    got = device_form(fe, name, X)
    bad = np.argwhere((got != want).any(axis=1)).ravel()
    assert bad.size == 0, (name, len(bad), [(int(j), got[j].tolist(), want[j].tolist()) for j in bad[:2]])


@pytest.mark.parametrize("name", fc.HELPERS)
def test_helper_matches_model(fe, tables, name):
    iw, ow, X = fc.helper_inputs(name, random.Random(name))
    want = fc.helper_model(name, X, fc.consts_of(tables[0])).astype(np.uint32)
    inp = np.ascontiguousarray(X.astype(np.uint32))
    out = np.zeros((X.shape[0], ow), np.uint32)
    assert fe.fe_helper(name.encode(), _p(inp), iw, _p(out), ow, X.shape[0]) == 0
    bad = np.argwhere((out != want).any(axis=1)).ravel()
    assert bad.size == 0, (name, len(bad), [(int(j), out[j].tolist(), want[j].tolist()) for j in bad[:2]])


def test_uniform_constants_per_block(fe, tables):
    """one launch, the same lanes in every block, a different constant set in each neighbouring block: each block's
    result is its own constants' (a per-lane or a lane-0 read of the constants would mix them up)"""
    rng = random.Random(0xB10C)
    for name in ("dot3_uc", "dot4_uc", "dot2_add_uc_narrow", "mul_uc_narrow", "mul_uc_add_narrow", "mul_vv_adds_narrow"):
        doms = fc.DOMAINS[name]
        lanes = np.stack([fc.random_limbs(rng, d, fc.BLOCK) if d != fc.CONST else np.zeros((fc.BLOCK, NL), np.uint64)
                          for d in doms], axis=1)
        nblk = 16
        X = np.concatenate([lanes] * nblk)
        for b in range(nblk):
            for s, d in enumerate(doms):
                if d == fc.CONST:
                    X[b * fc.BLOCK:(b + 1) * fc.BLOCK, s] = fm.to_limbs(rng.randrange(P))
        X = X[: nblk * fc.BLOCK - 5]
        want = fc.model(name, X)[0].astype(np.uint32)
        got = device_form(fe, name, X)
        assert (got == want).all(), name
        assert len({tuple(got[b * fc.BLOCK]) for b in range(nblk)}) == nblk, name


def device_permute(fe, quad, X):
    inp = np.ascontiguousarray(X.astype(np.uint32))
    out = np.full(inp.shape, 0xFFFFFFFF, np.uint32)
    assert fe.fe_permute(quad, _p(inp), _p(out), X.shape[0]) == 0
    return out.astype(np.uint64)


def test_thread_permute_from_noncanonical_entries(fe, emul, oracle):
    """permute() at its entry bounds (lane 0 < 32p, lanes 1, 2 < 16p, top limbs at the maximum): the oracle on the
    reduced values, the host build of the same schedule bit for bit, the exit bounds on the raw lanes"""
    X = entry_states(4099, 0x7E)
    got = device_permute(fe, 0, X)
    assert (got == host_permute(emul, X)).all()
    check_exit(oracle, X[:1500], got[:1500])


def test_quad_permute_from_noncanonical_entries(fe, oracle):
    """coop::permute from entries below 32p on every lane (tests/test_fe_forms.py::test_coop_schedule_bounds):
    the oracle on the reduced values; exit lanes normalised and below 1.02p"""
    rng = random.Random(0xC0)
    b = 32 * P
    X = np.concatenate([np.array([[fc.max_limbs(W, b)] * 3, [fm.to_limbs(b - 1)] * 3, [fm.to_limbs(0)] * 3,
                                  [fm.to_limbs(31 * P + 1), fm.to_limbs(P), fm.to_limbs(P - 1)]], np.uint64),
                        np.stack([fc.random_limbs(rng, (W, b), 1500) for _ in range(3)], axis=1)])
    got = device_permute(fe, 1, X)
    rinv = pow(fm.R, -1, P)
    for j in range(X.shape[0]):
        s = [x * rinv % P for x in fm.ints(X[j])]
        e = fm.ints(got[j])
        assert [x * rinv % P for x in e] == oracle.permute(s), j
        assert max(e) < 102 * P // 100 and (got[j][:, :NL - 1] < 1 << W).all(), (j, [x / P for x in e])
