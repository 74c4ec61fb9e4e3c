"""CPU: the recurrence schedule of csrc/imt_device.hpp::permute -- its generated assembly form (csrc/imt_mont_asm_rec.hpp)
and the worst-case value bounds of the partial rounds' window, their exit and the full rounds around them."""
import os
import subprocess
import sys
from fractions import Fraction

from oracle_lib import P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
NL = 9
P29 = [(P >> (29 * i)) & ((1 << 29) - 1) for i in range(NL)]

# v_mad_u64_u32 per form of csrc/imt_mont_asm_rec.hpp: 4 x 81 limb products, 81 digit products, 8 addend limbs as mad(e, 1)
REC_MAD_COUNTS = {"dot4_add_uc": 324 + 81 + 8}


def test_generated_recurrence_header_is_current(tmp_path):
    """csrc/imt_mont_asm_rec.hpp is what `gen_mont_asm.py --rec` writes, and holds exactly its forms and mads."""
    out = tmp_path / "imt_mont_asm_rec.hpp"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_mont_asm.py"), "--rec", str(out)], check=True,
                   stdout=subprocess.DEVNULL)
    committed = open(os.path.join(CSRC, "imt_mont_asm_rec.hpp")).read()
    assert out.read_text() == committed
    blocks = committed.split("__device__ __forceinline__ void ")[1:]
    assert sorted(b.split("(")[0] for b in blocks) == sorted(REC_MAD_COUNTS)
    for b in blocks:
        name = b.split("(")[0]
        assert b.count('"v_mad_u64_u32') == REC_MAD_COUNTS[name]
        assert b.count('"v_mul_lo_u32') == NL                   # wide digits: no mask per digit
        assert "v_and_b32_e32 %[r" not in b.split("v_lshrrev_b64")[0]
        for line in b.splitlines():                              # vector instructions only
            if line.strip().startswith('"'):
                assert line.strip()[1:].startswith("v_"), line


def test_dot4_add_column_budget():
    """The 4-term form with wide digits and a per-lane addend: every column accumulator stays below 2^64 when every
    multiplicand limb is below 2^29 (constants < p; window values normalised, < 2^261) and the addend limbs are too."""
    lim = (1 << 29) - 1
    carry = 0
    peak = 0
    for k in range(2 * NL - 1):
        lo, hi = max(0, k - (NL - 1)), min(k, NL - 1)
        acc = carry + 4 * (hi - lo + 1) * lim * lim                               # a[t][i] * b[t][k - i]
        acc += sum(((1 << 32) - 1) * P29[k - i] for i in range(max(0, k - (NL - 1)), min(k, NL - 1) + 1))   # m_i p_k-i
        if k >= NL:
            acc += lim                                                           # addend limb k - 9
        assert acc < 1 << 64, k
        peak = max(peak, acc)
        carry = acc >> 29
    assert carry + lim < 1 << 32                                                 # top limb: v_add of the last addend limb
    assert Fraction(peak, 1 << 64) < Fraction(99, 100)


def test_recurrence_schedule_bounds():
    """Worst-case proof, in units of p, for permute(): every S-box operand, every window value of the recurrence and
    every product stays a valid multiplicand (< 2^261, top limb < 2^29), the S-box inputs are lazy sums of two
    normalised values (limbs < 2^30), and the exit bounds close the loop over the sponge's two permutations and
    canonicalize (< 32p)."""
    rho = Fraction(P, 1 << 261)                 # p / R
    cap = 1 / rho                               # 2^261 in units of p
    worst = Fraction(0)

    def see(*xs):
        nonlocal worst
        for x in xs:
            assert x < cap
            worst = max(worst, x)

    def up(x):
        return Fraction(-((-x.numerator << 32) // x.denominator), 1 << 32)

    def red(t, wide=True, addend=Fraction(0)):   # REDC of products bounded by t p^2, plus addend * R
        return up(t * rho + addend + (8 if wide else 1))

    def sbox(x):                                # x: lane + constant (< p)
        x2 = red(x * x)
        x4 = red(x2 * x2)
        y = red(x4 * x)
        see(x, x2, x4, y)
        return y

    def full(lanes, ones_row):
        y = [sbox(v + 1) for v in lanes]
        n0 = sum(y) if ones_row else red(sum(y))
        n = [n0, red(sum(y)), red(sum(y))]      # matrix entries < p
        see(*n)
        return n

    def permute(lanes):
        for f in range(4):
            lanes = full(lanes, f != 0)
        a, b, z3, z2 = lanes[0], lanes[1], Fraction(0), lanes[2]
        for r in range(57):
            z = sbox(a + 1)                     # a + rec_k: both normalised
            if r >= 2:
                w = red(a + b + z3 + z2, addend=z)                 # dot4_add_uc, wide digits
            elif r == 1:
                w = red(a + z2, wide=False, addend=z3 + z)        # dot2_add_uc_narrow
            else:
                w = b + z                                          # lazy add + normalize
            see(w)
            a, b, z3, z2 = w, a, z2, z
        lanes = [a] + [red(a + b + z3, addend=z2)] * 2             # dot3_uc + z_56, normalize
        see(*lanes)
        for f in range(4):
            lanes = full(lanes, f != 0)
        return lanes

    entry = [Fraction(32), Fraction(16), Fraction(16)]
    out = permute(entry)
    assert out[0] < 32                          # the capacity lane enters the next permutation / canonicalize
    assert out[1] < 9 and out[2] < 9            # + an absorbed input or the padding 1: < 16p at the next entry
    assert worst < 120                          # headroom to 2^261 = 169.4p
