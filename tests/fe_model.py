"""Reference model of the device field arithmetic (csrc/imt_device.hpp, csrc/imt_trace_device.hpp), limb for limb.

A literal restatement, vectorised over numpy rows, of the column algorithm of mont_dot<NT, ADD, WIDE_M>, mont_sqr
and mont_redc, and of the helpers the products feed into.  Limbs are uint64 arrays [n, 9] holding 32-bit values;
every 64-bit sum wraps the way the device's does, and each accumulator's true peak is tracked (a carry out of bit
63 is reported as overflow), so a test can compare a kernel's raw output limbs and not only its residue mod p.

FORMS maps each assembly form of csrc/imt_mont_asm.hpp (tools/gen_mont_asm.py) to the C++ form it replaces, as the
`#else` branches of its call sites read:
  mul_vv              mont_dot<1, false, true>    mont_mul (S-box, load_fe / store_fe)
  sqr_v               mont_sqr                    sbox
  dot3_uc, dot4_uc    mont_dot<3|4, false, true>  permute's rows; first factors uniform table constants
  dot2_add_uc_narrow  mont_dot<2, true, false>    permute's s2 update; first factors uniform
  sqr_v_narrow        mont_dot<1, false, false>(a, a)   t_sqr; the coop S-box
  mul_vv_adds_narrow  mont_dot<1, true, false>    t_mul_add; the addend uniform
  mul_uc_narrow       mont_dot<1, false, false>   t_mulc; first factor uniform
  mul_uc_add_narrow   mont_dot<1, true, false>    t_mulc_add; first factor uniform
  redc_v_narrow       mont_redc                   t_emit (canonical output)
  mul_vv_narrow, mul_vv_add_narrow, dot3_vv_narrow  mont_dot<1|1|3, false|true|false, false>  the coop schedule
"""
from collections import namedtuple

import numpy as np

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
NL, W = 9, 29
MASK = (1 << W) - 1
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
R = 1 << 261
PL = [(P >> (W * i)) & MASK for i in range(NL)]
N0INV29 = (-pow(P, -1, 1 << 29)) % (1 << 29)
N0INV32 = (-pow(P, -1, 1 << 32)) % (1 << 32)
assert N0INV29 == 0x0FFFFFFF and N0INV32 == 0xEFFFFFFF

# kind: "dot" (mont_dot), "sqr" (mont_sqr), "redc" (mont_redc).  uniform: which operand the assembly takes from SGPRs
# ("a" = the first factor of every term, "e" = the addend).
Form = namedtuple("Form", "kind nt add wide uniform")
FORMS = {
    "mul_vv": Form("dot", 1, False, True, None),
    "sqr_v": Form("sqr", 1, False, True, None),
    "dot3_uc": Form("dot", 3, False, True, "a"),
    "dot4_uc": Form("dot", 4, False, True, "a"),
    "dot2_add_uc_narrow": Form("dot", 2, True, False, "a"),
    "sqr_v_narrow": Form("dot", 1, False, False, None),          # mont_dot(a, a): the operand is used twice
    "mul_vv_adds_narrow": Form("dot", 1, True, False, "e"),
    "mul_uc_narrow": Form("dot", 1, False, False, "a"),
    "mul_uc_add_narrow": Form("dot", 1, True, False, "a"),
    "redc_v_narrow": Form("redc", 0, False, False, None),
    "mul_vv_narrow": Form("dot", 1, False, False, None),
    "mul_vv_add_narrow": Form("dot", 1, True, False, None),
    "dot3_vv_narrow": Form("dot", 3, False, False, None),
}
SQUARES = ("sqr_v", "sqr_v_narrow")


def operands(name):
    """Operand slots of a form in call order: ("a", t), ("b", t) for each term, then ("e", 0) for the addend.
    A squaring or a REDC has the single slot ("a", 0)."""
    f = FORMS[name]
    if f.kind != "dot" or name in SQUARES:
        return [("a", 0)]
    return [(s, t) for t in range(f.nt) for s in "ab"] + ([("e", 0)] if f.add else [])


# ---- integers <-> limbs ----------------------------------------------------------------------------------------------
def to_limbs(x):
    """normalised limbs: eight 29-bit digits, the top limb holds the rest (must fit 32 bits)"""
    assert 0 <= x < 1 << (W * 8 + 32)
    return [(x >> (W * i)) & MASK for i in range(NL - 1)] + [x >> (W * (NL - 1))]


def from_limbs(l):
    return sum(int(v) << (W * i) for i, v in enumerate(l))


def arr(rows):
    """list of 9-limb lists -> uint64 [n, 9]"""
    return np.array(rows, dtype=np.uint64).reshape(-1, NL)


def ints(a):
    """uint [n, 9] limbs -> list of Python ints (limbs weighted by 2^29, not necessarily normalised)"""
    a = np.asarray(a, dtype=object)
    out = a[:, 0].copy()
    for i in range(1, NL):
        out = out + (a[:, i] << (W * i))
    return list(out)


def words_to_int(w):
    a = np.asarray(w, dtype=object)
    out = a[:, 0].copy()
    for i in range(1, a.shape[1]):
        out = out + (a[:, i] << (32 * i))
    return list(out)


# ---- the products ----------------------------------------------------------------------------------------------------
class _Acc:
    """A column accumulator: uint64 with wrap-around, plus the carry-out flag and the peak over column ends."""

    def __init__(self, n):
        self.v = np.zeros(n, np.uint64)
        self.ovf = np.zeros(n, bool)
        self.peak = np.zeros(n, np.uint64)

    def add(self, x):
        s = self.v + x
        self.ovf |= s < self.v
        self.v = s

    def mad(self, x, y):
        self.add(x * y)        # x, y < 2^32: the product is exact in 64 bits

    def end(self):             # every term is non-negative: a column's sum peaks at its end
        self.peak = np.maximum(self.peak, self.v)


def _digit(lo, wide):
    lo = lo & np.uint64(M32)
    if wide:
        return (lo * np.uint64(N0INV32)) & np.uint64(M32)
    return (lo * np.uint64(N0INV29)) & np.uint64(MASK)


def mont(name, a, b=None, e=None):
    """One form on rows.  a, b: uint64 [nt, n, 9] (a [n, 9] for a squaring / REDC); e: the addend [n, 9].
    Returns (r [n, 9] uint64 holding 32-bit limbs, peak [n] uint64, overflow [n] bool)."""
    f = FORMS[name]
    with np.errstate(over="ignore"):
        if f.kind == "dot" and name in SQUARES:       # sqr_v_narrow: mont_dot<1, false, false>(a, a)
            a = np.asarray(a, np.uint64)[None]
            b = a
        elif f.kind == "dot":
            a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
        else:
            a = np.asarray(a, np.uint64)
        n = a.shape[-2]
        acc = _Acc(n)
        m = [None] * NL
        r = np.zeros((n, NL), np.uint64)
        p = [np.uint64(x) for x in PL]
        sh = np.uint64(W)
        if f.kind == "sqr":
            a2 = (a << np.uint64(1)) & np.uint64(M32)

        def products(k):
            lo, hi = max(0, k - (NL - 1)), min(k, NL - 1)
            if f.kind == "redc":
                if k < NL:
                    acc.add(a[:, k])
            elif f.kind == "sqr":
                for i in range(lo, hi + 1):
                    if 2 * i < k:
                        acc.mad(a2[:, i], a[:, k - i])
                if k % 2 == 0:
                    acc.mad(a[:, k // 2], a[:, k // 2])
            else:
                for t in range(a.shape[0]):
                    for i in range(lo, hi + 1):
                        acc.mad(a[t][:, i], b[t][:, k - i])

        wide = f.wide
        for k in range(NL):
            products(k)
            for i in range(k):
                acc.mad(m[i], p[k - i])
            m[k] = _digit(acc.v, wide)
            acc.mad(m[k], p[0])
            acc.end()
            acc.v = acc.v >> sh
        for k in range(NL, 2 * NL - 1):
            products(k)
            for i in range(k - (NL - 1), NL):
                acc.mad(m[i], p[k - i])
            if f.add:
                acc.add(np.asarray(e, np.uint64)[:, k - NL])
            acc.end()
            r[:, k - NL] = acc.v & np.uint64(MASK)
            acc.v = acc.v >> sh
        if f.add:
            acc.add(np.asarray(e, np.uint64)[:, NL - 1])
        r[:, NL - 1] = acc.v & np.uint64(M32)
    return r, acc.peak, acc.ovf


def mont_value(name, a, b=None, e=None):
    """What a form computes, as integers: (T, add) with r = (T + m p) / R + add, i.e. r = T R^-1 + add mod p and
    r < T / R + add + (8p if wide else p).  Same argument shapes as mont()."""
    f = FORMS[name]
    if f.kind == "redc":
        return ints(a), [0] * len(ints(a))
    if name in SQUARES:
        x = ints(a)
        return [v * v for v in x], [0] * len(x)
    T = [0] * np.asarray(a).shape[1]
    for t in range(np.asarray(a).shape[0]):
        T = [s + x * y for s, x, y in zip(T, ints(a[t]), ints(b[t]))]
    return T, (ints(e) if f.add else [0] * len(T))


# ---- the helpers ----------------------------------------------------------------------------------------------------
def p_shl(sh):
    """limbs of p << sh as p29_shl<SH> lays them out (normalised, top limb whatever is left)"""
    return to_limbs(P << sh)


def normalize(a):
    a = np.array(a, np.uint64)
    for i in range(NL - 1):
        a[:, i + 1] = (a[:, i + 1] + (a[:, i] >> np.uint64(W))) & np.uint64(M32)
        a[:, i] &= np.uint64(MASK)
    return a


def _sub_shl(a, sh):
    """a - (p << sh) with the borrow chain of cond_sub_p_shl / csub (u32 arithmetic), and the final borrow word"""
    ps = p_shl(sh)
    a = np.asarray(a, np.int64)
    d = np.zeros_like(a)
    borrow = np.zeros(a.shape[0], np.int64)
    for i in range(NL):
        x = (a[:, i] - ps[i] - borrow) & M32
        if i < NL - 1:
            borrow = x >> 31
            d[:, i] = x & MASK
        else:
            d[:, i] = x
    return d.astype(np.uint64)


def cond_sub_p_shl(a, sh):
    """a -= (p << sh) if a >= (p << sh), by the limb-wise compare of imt_device.hpp"""
    a = np.asarray(a, np.uint64)
    ps = p_shl(sh)
    ge = np.ones(a.shape[0], bool)
    for i in range(NL):
        ne = a[:, i] != np.uint64(ps[i])
        ge = np.where(ne, a[:, i] > np.uint64(ps[i]), ge)
    return np.where(ge[:, None], _sub_shl(a, sh), a)


def canonicalize(a):
    for sh in (4, 3, 2, 1, 0):
        a = cond_sub_p_shl(a, sh)
    return a


def csub(a, sh):
    """imt_trace_device.hpp::csub<SH>: keep a where the top limb of a - (p << sh) went negative (as int32)"""
    a = np.asarray(a, np.uint64)
    d = _sub_shl(a, sh)
    keep = d[:, NL - 1].astype(np.uint32).view(np.int32) < 0
    return np.where(keep[:, None], a, d)


def t_add(a, b):
    s = (np.asarray(a, np.uint64) + np.asarray(b, np.uint64)) & np.uint64(M32)
    return csub(normalize(s), 1)


FOLD_RECIP = 1354
PC = [(1 << 29) - PL[0]] + [MASK - PL[i] for i in range(1, NL)]      # limbs of 2^261 - p


def fold_p(a):
    a = np.asarray(a, np.uint64)
    with np.errstate(over="ignore"):
        q = (a[:, NL - 1] * np.uint64(FOLD_RECIP)) >> np.uint64(32)
        acc = np.zeros(a.shape[0], np.uint64)
        r = np.zeros_like(a)
        for i in range(NL):
            acc = (acc >> np.uint64(W)) + a[:, i] + q * np.uint64(PC[i])
            if i < NL - 1:
                r[:, i] = acc & np.uint64(MASK)
            else:
                r[:, i] = (acc - (q << np.uint64(W))) & np.uint64(M32)
    return r


def unpack(w):
    """8 x u32 words -> nine 29-bit limbs"""
    w = np.asarray(w, np.uint64)
    r = np.zeros((w.shape[0], NL), np.uint64)
    for i in range(NL):
        bit = W * i
        wi, sh = bit >> 5, bit & 31
        lo = w[:, wi] >> np.uint64(sh)
        if sh > 3 and wi + 1 < 8:
            lo |= (w[:, wi + 1] << np.uint64(32 - sh)) & np.uint64(M32)
        r[:, i] = lo & np.uint64(MASK)
    return r


def pack(a):
    """nine limbs -> 8 x u32 words, as imt_device.hpp::pack (u32 shifts: bits above 32 are dropped)"""
    a = np.asarray(a, np.uint64)
    w = np.zeros((a.shape[0], 8), np.uint64)
    for j in range(8):
        lo_limb = (32 * j) // W
        off = 32 * j - W * lo_limb
        x = a[:, lo_limb] >> np.uint64(off)
        have = W - off
        if have < 32 and lo_limb + 1 < NL:
            x |= (a[:, lo_limb + 1] << np.uint64(have)) & np.uint64(M32)
        if have + W < 32 and lo_limb + 2 < NL:
            x |= (a[:, lo_limb + 2] << np.uint64(have + W)) & np.uint64(M32)
        w[:, j] = x & np.uint64(M32)
    return w


def geq_p(a):
    a = np.asarray(a, np.uint64)
    ge = np.ones(a.shape[0], bool)
    for i in range(NL):
        ne = a[:, i] != np.uint64(PL[i])
        ge = np.where(ne, a[:, i] > np.uint64(PL[i]), ge)
    return ge


def _times(a, c_limbs):
    c = np.broadcast_to(np.asarray(c_limbs, np.uint64), np.asarray(a).shape)
    return mont("mul_vv", np.asarray(a, np.uint64)[None], c[None])[0]


def load_fe(w, fmt, consts):
    """load_fe(pc, r, words, fmt): (limbs, ok).  consts: the PoseidonConsts entries by name (limb lists)"""
    raw = unpack(w)
    ok = ~geq_p(raw) & ((raw[:, NL - 1] >> np.uint64(24)) == 0)
    if fmt == 2:
        return raw, ok
    r = _times(raw, consts["from_canon"] if fmt == 0 else consts["from_mont256"])
    return canonicalize(r), ok


def store_fe(a, fmt, consts):
    if fmt == 2:
        return pack(a)
    t = _times(a, consts["int_one"] if fmt == 0 else consts["to_mont256"])
    return pack(canonicalize(t))


def _top_limb_of_multiple(k):
    acc = 0
    for i in range(NL):
        acc = (acc >> W) + k * PL[i]
    return acc & M32


def store_mont256(a):
    """imt_trace_device.hpp::store_mont256 on rows of nine limbs (value < 4p): the eight words it stores"""
    a = np.asarray(a, np.uint64).astype(np.int64)
    n = a.shape[0]
    m = (-a[:, 0]) & 31
    q = {31: _top_limb_of_multiple(1), 30: _top_limb_of_multiple(2), 29: _top_limb_of_multiple(3)}
    q8 = np.full(n, M32, np.int64)
    for mm, v in q.items():
        q8 = np.where(m == mm, v, q8)
    neg = a[:, NL - 1] > q8
    s = np.zeros(n, np.int64)
    for i in range(NL):
        s = (s >> W) + a[:, i] + (m - 32) * PL[i]
    neg = np.where(a[:, NL - 1] == q8, s >= 0, neg)
    ms = m - np.where(neg, 32, 0)
    w = np.zeros((n, 8), np.uint64)
    acc = (a[:, 0] + ms * PL[0]) >> 5
    for j in range(8):
        sh = 24 - 3 * j
        acc = acc + (a[:, j + 1] << sh) + (ms * (1 << sh)) * PL[j + 1]
        w[:, j] = (acc & M32).astype(np.uint64)
        acc = acc >> 32
    return w
