"""CPU: the Montgomery forms and helpers of the device arithmetic, limb for limb.

tests/fe_model.py restates the column algorithm of mont_dot / mont_sqr / mont_redc; here it is checked bit for bit
against the host build of the C++ forms on each form's operand corpus (tests/fe_corpus.py), and every corpus row is
checked for what the callers rely on: the residue, the value bound (+8p wide, +p narrow), normalised output limbs and a
column peak below 2^64.  Then: the thread-per-hash permutation from non-canonical entries at its documented bounds,
the worst-case value bounds of the coop (quad-lane) and witness-trace schedules, and the gfx950 assembly of the GPU
harness (tests/native/fe_forms.hip), which must hold each form's exact v_mad_u64_u32 count and, for the forms with
uniform operands, no v_readfirstlane."""
import ctypes
import os
import random
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fe_corpus as fc
import fe_model as fm
from fe_model import NL, P, R, W
from test_host_logic import MAD_COUNTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.environ.get("FE_FORMS_CSRC") or os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
FORM_NAMES = list(fm.FORMS)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def tables(emul):
    n = emul.emul_consts_size() // 4
    buf = np.zeros(n, np.uint32)
    emul.emul_consts_raw(_p(buf))
    pc = fc.parse(buf, fc.PC_LAYOUT)
    n = emul.emul_trace_consts_size() // 4
    buf = np.zeros(n, np.uint32)
    emul.emul_trace_consts_raw(_p(buf))
    return pc, fc.parse(buf, fc.TC_LAYOUT)


def host_form(emul, name, X):
    inp = np.ascontiguousarray(X.astype(np.uint32))
    out = np.zeros((X.shape[0], NL), np.uint32)
    assert emul.emul_form(FORM_NAMES.index(name), _p(inp), _p(out), ctypes.c_size_t(X.shape[0])) == 0
    return out


def analytic_peak(name):
    """the worst column sum allowed by the slot widths: a*b part + m*p part (each limb of p once per column, digits
    below 2^32 or 2^29) + the carry in (< 2^36) + the addend limb"""
    f = fm.FORMS[name]
    doms = fc.DOMAINS[name]
    width = [W if d == fc.CONST else d[0] for d in doms]
    lim = [(1 << w) - 1 for w in width]
    m_max = (1 << 32) - 1 if f.wide else (1 << W) - 1
    worst = 0
    for k in range(2 * NL - 1):
        lo, hi = max(0, k - (NL - 1)), min(k, NL - 1)
        if f.kind == "redc":
            ab = lim[0] if k < NL else 0
        elif name in fm.SQUARES:
            cross = len([i for i in range(lo, hi + 1) if 2 * i < k])
            ab = cross * ((lim[0] << 1) * lim[0]) + (lim[0] ** 2 if k % 2 == 0 else 0)
        else:
            ab = f.nt * (hi - lo + 1) * max(lim[2 * t] * lim[2 * t + 1] for t in range(f.nt))
        mp = sum(m_max * fm.PL[k - i] for i in range(lo, hi + 1))
        add = lim[-1] if f.add and k >= NL else 0
        worst = max(worst, ab + mp + (1 << 36) + add)
    return worst


@pytest.mark.parametrize("name", FORM_NAMES)
def test_model_matches_host_forms(emul, tables, name):
    X = fc.corpus(name, *tables)
    r, _, ovf = fc.model(name, X)
    assert not ovf.any()
    got = host_form(emul, name, X)
    bad = np.argwhere((got != r.astype(np.uint32)).any(axis=1))
    assert bad.size == 0, (name, bad[:4].ravel().tolist())


@pytest.mark.parametrize("name", FORM_NAMES)
def test_form_corpus_semantics(tables, name):
    """residue, value bound, normalised limbs and column peak on every corpus row"""
    f = fm.FORMS[name]
    X = fc.corpus(name, *tables)
    r, peak, ovf = fc.model(name, X)
    assert not ovf.any() and int(peak.max()) < 1 << 64
    assert int(peak.max()) <= analytic_peak(name) < 1 << 64
    assert (r[:, :NL - 1] < 1 << W).all()
    T, add = fm.mont_value(name, *fc.split(name, X))
    T = np.array(T, dtype=object)
    add = np.array(add, dtype=object)
    rv = np.array(fm.ints(r), dtype=object)
    assert (((rv - add) * R - T) % P == 0).all(), name
    slack = 8 * P if f.wide else P
    assert ((rv - add - slack) * R < T).all(), name
    # the domain really is what the corpus claims: every slot inside its width and bound
    for s, dom in enumerate(fc.DOMAINS[name]):
        width, bound = (W, P) if dom == fc.CONST else dom
        assert (X[:, s, :NL - 1] < 1 << width).all() and (X[:, s, NL - 1] < 1 << width).all()
        assert max(fm.ints(X[:, s])) < bound


def test_form_peaks_reach_their_corners(tables):
    """the peak search gets within reach of the analytic bound: the corpus exercises the carry-heavy columns"""
    for name in FORM_NAMES:
        peak = int(fc.model(name, fc.corpus(name, *tables))[1].max())
        assert peak > 0.8 * analytic_peak(name), name


@pytest.mark.parametrize("name", fc.HELPERS)
def test_helper_model_matches_host(emul, tables, name):
    iw, ow, X = fc.helper_inputs(name, random.Random(name))
    want = fc.helper_model(name, X, fc.consts_of(tables[0])).astype(np.uint32)
    inp = np.ascontiguousarray(X.astype(np.uint32))
    out = np.zeros((X.shape[0], ow), np.uint32)
    assert emul.emul_helper(name.encode(), _p(inp), iw, _p(out), ow, ctypes.c_size_t(X.shape[0])) == 0
    bad = np.argwhere((out != want).any(axis=1))
    assert bad.size == 0, (name, bad[:4].ravel().tolist())


def test_helper_values(tables):
    """what the callers rely on from the helpers, on their corpora"""
    rng = random.Random(7)
    _, _, X = fc.helper_inputs("canonicalize", rng)
    v, c = fm.ints(X), fm.ints(fm.canonicalize(X))
    assert all(y == x % P for x, y in zip(v, c))
    _, _, X = fc.helper_inputs("fold_p", rng)
    v, f = fm.ints(X), fm.ints(fm.fold_p(X))
    assert all(y % P == x % P and y < Fraction(6, 5) * P for x, y in zip(v, f))
    _, _, X = fc.helper_inputs("t_add", rng)
    s = fm.ints(fm.t_add(X[:, :9], X[:, 9:]))
    assert all(y % P == (a + b) % P and y < Fraction(11, 5) * P
               for a, b, y in zip(fm.ints(X[:, :9]), fm.ints(X[:, 9:]), s))
    _, _, X = fc.helper_inputs("store_mont256", rng)
    w = fm.words_to_int(fm.store_mont256(X))
    inv32 = pow(32, -1, P)
    assert all(y == x * inv32 % P for x, y in zip(fm.ints(X), w))


# ---- the thread-per-hash permutation from raw entries ------------------------------------------------------------------
def entry_states(n, seed):
    """raw entry lanes at permute()'s documented bounds: lane 0 < 32p, lanes 1, 2 < 16p, normalised limbs"""
    rng = random.Random(seed)
    b = [32 * P, 16 * P, 16 * P]
    rows = [[fc.max_limbs(W, x) for x in b], [fm.to_limbs(x - 1) for x in b], [fm.to_limbs(0)] * 3,
            [fm.to_limbs(31 * P), fm.to_limbs(15 * P + 1), fm.to_limbs(15 * P - 1)]]
    rows += [[fm.to_limbs(rng.choice([k * P - 1, k * P, k * P + 1, rng.randrange(x)]) % x)
              for x in b for k in [rng.randrange(1, x // P + 1)]] for _ in range(n // 2)]
    lanes = [fc.random_limbs(rng, (W, x), n - len(rows)) for x in b]
    rows = np.concatenate([np.array(rows, np.uint64), np.stack(lanes, axis=1)])
    for l, x in enumerate(b):
        assert max(fm.ints(rows[:, l])) < x
    return rows


def check_exit(oracle, entry, exit_, rinv=pow(R, -1, P)):
    """exit lanes against the oracle on the reduced entry values; raw exit bounds: lane 0 < 30p, lanes 1, 2 < 9p"""
    for j in range(entry.shape[0]):
        s = [x * rinv % P for x in fm.ints(entry[j])]
        e = fm.ints(exit_[j])
        assert [x * rinv % P for x in e] == oracle.permute(s), j
        assert e[0] < 30 * P and e[1] < 9 * P and e[2] < 9 * P, (j, [x / P for x in e])
        assert (exit_[j][:, :NL - 1] < 1 << W).all()


def host_permute(emul, X):
    inp = np.ascontiguousarray(X.astype(np.uint32))
    out = np.zeros_like(inp)
    emul.emul_permute_raw(_p(inp), _p(out), ctypes.c_size_t(X.shape[0]))
    return out.astype(np.uint64)


def test_thread_permute_from_noncanonical_entries(emul, oracle):
    X = entry_states(3000, 0xE17)
    check_exit(oracle, X, host_permute(emul, X))


# ---- worst-case proofs of the other two schedules ----------------------------------------------------------------------
RHO = Fraction(P, R)          # p / R: a product of bounds a p and b p contributes a b RHO p after REDC
CAP = 1 / RHO                 # 2^261 in units of p


def _up(x):
    return Fraction(-((-x.numerator << 32) // x.denominator), 1 << 32)


def test_coop_schedule_bounds():
    """imt_coop_device.hpp::permute, in units of p, all products with 29-bit digits (REDC(T) < T / R + p): every operand
    stays below the corpus bound fc.COOP (< 2^261); the linear lanes grow by < 1.01p per partial round; the exit lanes
    close the loop over the sponge's two permutations (entry + an absorbed canonical input) and canonicalize (< 32p)."""
    worst, growth = Fraction(0), Fraction(0)

    def see(*xs):
        nonlocal worst
        for x in xs:
            assert x < CAP
            worst = max(worst, x)

    def red(t):
        return _up(t * RHO + 1)

    def permute(S):
        for st in range(65):
            if st < 4 or st >= 61:
                ys = []
                for s in S:                     # v = S + k (lazy); x^2, x^4, x^5 -- one lane each
                    v = s + 1
                    x2 = red(v * v)
                    x4 = red(x2 * x2)
                    y = red(x4 * v)
                    see(v, x2, x4, y)
                    ys.append(y)
                S = [red(sum(ys))] * 3          # dot3_vv_narrow(M row, Y), entries < p
                see(*S)
            else:
                nonlocal growth
                v = S[0] + 1                    # x = s0 + k on lanes 0 and 3, broadcast
                e1_0, e1_c = red(v * v), red(v)     # lane 0: x^2; lanes 1, 2: col x; lane 3: row0 x
                x4 = red(e1_0 * e1_0)
                u = [red(S[1]), red(S[2])]      # lanes 1, 2: row_i s_i
                add = u[0] + u[1]
                step = red(x4 * e1_c)           # x^4 (col x) or x^4 (row0 x)
                S = [step + add, S[1] + step, S[2] + step]
                growth = max(growth, step)
                see(v, e1_0, e1_c, x4, *u, add, *S)
        return S

    entry = Fraction(32)                        # any lane below 32p: what canonicalize accepts
    out = permute([entry] * 3)
    assert max(out) + 1 < entry                 # second permutation: + c or the padding 1 (canonical)
    assert max(permute([max(out) + 1] * 3)) < 32    # canonicalize on lane 1
    assert growth < Fraction(101, 100)
    assert worst * P < fc.COOP                  # the corpus covers every operand of the schedule


def test_trace_schedule_bounds():
    """imt_trace_device.hpp::permute_trace, in units of p, 29-bit digits throughout: every operand and every emitted
    value stays below 4p (fc.TRACE, store_mont256's and t_emit's precondition) over both permutations of a hash."""
    worst = Fraction(0)

    def see(*xs):
        nonlocal worst
        for x in xs:
            worst = max(worst, x)

    def red(t):
        return _up(t * RHO + 1)

    def red2(x):                                # csub<1>: a - 2p where a >= 2p
        assert x < 6
        return max(min(x, Fraction(2)), x - 2)

    def t_add(a, b):
        assert a < Fraction(16, 5) and b <= 1   # t_add's documented precondition
        r = red2(a + b)
        see(r)
        return r

    def x5c(x):
        x2 = red(x * x)
        x4 = red(x2 * x2)
        y = red(x * x4) + 1                     # + the uniform constant (< p)
        see(x, x2, x4, y)
        return y

    def inner(s):
        a0 = red(s[0])
        a1 = red(s[1]) + a0
        r = red(s[2]) + a1
        see(a0, a1, r)
        return r

    def permute(s, n_in):
        s = list(s)
        s[0] = t_add(s[0], 1)
        if n_in >= 1:
            s[1] = t_add(s[1], 1)
        s[1] = t_add(s[1], 1)
        if n_in >= 2:
            s[2] = t_add(s[2], 1)
        s[2] = t_add(s[2], 1)
        for st in range(65):
            if st < 4 or st >= 61:
                y = [x5c(v) for v in s]
                s = [inner(y)] * 3
            else:
                s0 = x5c(s[0])
                n0 = inner([s0, s[1], s[2]])
                s1 = red2(red(s0) + s[1])       # gate.mul_add(s0, col_hat, s_i), then red2
                s2 = red2(red(s0) + s[2])
                see(s1, s2)
                s = [n0, s1, s2]
        return s

    s = permute([Fraction(1)] * 3, 2)           # [2^64, 0, 0] canonical, inputs a, b
    for n_in in (0, 1):                         # the second permutation: hash2 (padding only) or hash3 (c)
        permute(s, n_in)
    assert worst * P < fc.TRACE


# ---- the harness's assembly ------------------------------------------------------------------------------------------
def _sgpr_first_factors(body):
    """v_mad_u64_u32 whose first factor (src0) is an SGPR: the uniform operands' products (the digits' m * p products
    take p as src1)"""
    return sum(l.split(",")[2].strip().startswith("s") for l in body.splitlines() if "v_mad_u64_u32" in l)


def test_harness_assembly(tmp_path):
    """each form's kernel holds exactly its form's v_mad_u64_u32 count (it runs the assembly, not the C++ fallback);
    the kernels with uniform operands hold no v_readfirstlane and take exactly their uniform factors from SGPRs.
    The "s" constraint does not force that: given a per-lane value the compiler keeps it in a VGPR (the instruction
    accepts either), so only the SGPR count shows a per-lane value at a uniform call site.  permute() calls the
    uniform forms from each of its code paths once: three 3-term rows per full round, a 3-term row, a 4-term row and
    the 2-term s2 update per partial-round pair."""
    out = tmp_path / "fe_forms.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC,
                    "--cuda-device-only", "-S", "-o", str(out), os.path.join(ROOT, "tests", "native", "fe_forms.hip")],
                   check=True, capture_output=True)
    asm = out.read_text()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(fe[khp]_\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm,
                                                          re.S | re.M)}
    for name in FORM_NAMES:
        f = fm.FORMS[name]
        b = bodies["fek_" + name]
        assert b.count("v_mad_u64_u32") == MAD_COUNTS[name], name
        uniform = {"a": 81 * f.nt, "e": NL - 1}.get(f.uniform, 0)     # the addend's top limb is a v_add, not a mad
        assert _sgpr_first_factors(b) == uniform, name
        if f.uniform:
            assert "v_readfirstlane" not in b, name
    # the helpers that multiply run mul_vv (load_fe / store_fe out of and into the canonical formats)
    for h in ("load_fe0", "load_fe1", "store_fe0", "store_fe1"):
        assert bodies["feh_" + h].count("v_mad_u64_u32") == MAD_COUNTS["mul_vv"], h
    b = bodies["fep_thread"]
    assert "v_readfirstlane" not in b
    assert _sgpr_first_factors(b) == 81 * (3 * 3 + 3 + 4 + 2)
