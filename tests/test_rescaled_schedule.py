"""CPU: the rescaled Poseidon schedule of csrc/imt_device.hpp::permute (lanes held divided by fifth roots of the
linear layer's constants) -- many states through the host build of the device code against the oracle, and the
worst-case value bounds of its lazily accumulated lane and its (1, 1, 1) rows."""
import ctypes
import random
from fractions import Fraction

from oracle_lib import P, b32


def _permute(emul, st):
    out = ctypes.create_string_buffer(96)
    assert emul.emul_permute(b"".join(map(b32, st)), out) == 0
    return [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(3)]


def _hash(emul, xs):
    out = ctypes.create_string_buffer(32)
    assert emul.emul_hash(b"".join(b32(x) for x in xs), len(xs), out, 0, 0) == 0
    return int.from_bytes(out.raw, "little")


def test_rescaled_permutation_matches_oracle(emul, oracle):
    rng = random.Random(0x5CA1ED)
    edge = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, 1 << 64, (1 << 253) - 1]
    states = [[x, x, x] for x in edge]                                     # all lanes equal
    states += [[a, b, c] for a in (0, P - 1) for b in (0, P - 1) for c in (0, P - 1)]
    states += [[rng.choice(edge) for _ in range(3)] for _ in range(200)]
    states += [[rng.randrange(P) for _ in range(3)] for _ in range(20000)]
    for st in states:
        assert _permute(emul, st) == oracle.permute(st), st


def test_rescaled_hash_matches_oracle(emul, oracle):
    rng = random.Random(0xBA5E)
    edge = [0, 1, P - 1, P - 2]
    cases = [[x] * n for x in edge for n in (2, 3)]
    cases += [[rng.choice(edge) for _ in range(rng.choice([2, 3]))] for _ in range(100)]
    cases += [[rng.randrange(P) for _ in range(rng.choice([2, 3]))] for _ in range(10000)]
    for c in cases:
        assert _hash(emul, c) == oracle.hash(c), c


def test_rescaled_schedule_bounds():
    """Worst-case proof, in units of p, for the lanes of permute(): every S-box operand and product stays a
    valid multiplicand (< 2^261: top limb < 2^29), the lazily added lane s1 stays below 2^261 between folds, the
    (1, 1, 1) row's sum fits, and the exit bounds close the loop over the sponge's two permutations and
    canonicalize (< 32p)."""
    rho = Fraction(P, 1 << 261)                 # p / R
    cap = 1 / rho                               # 2^261 in units of p
    worst = Fraction(0)

    def see(*xs):
        nonlocal worst
        for x in xs:
            assert x < cap
            worst = max(worst, x)

    def up(x):                                  # round a bound up to a multiple of 2^-32 (keeps the fractions small)
        return Fraction(-((-x.numerator << 32) // x.denominator), 1 << 32)

    def red(t, wide=True):                      # REDC of a sum of products bounded by t p^2
        return up(t * rho + (8 if wide else 1))

    def sbox(x):                                # x: lane + constant (< p)
        x2 = red(x * x)
        x4 = red(x2 * x2)
        y = red(x4 * x)
        see(x, x2, x4, y)
        return y

    # fold_p: q = floor(top * 1354 / 2^32) with 1354 = floor(2^264 / p), value < (top + 1) 2^232
    assert 1354 * P <= 1 << 264 < 1355 * P
    def fold(v):
        top = int(v * P) >> 232                 # largest top limb of a value below v p
        assert top < 1 << 29
        q_min = Fraction(top * 1354, 1 << 32) - 1
        return up(Fraction((top + 1) << 232, P) - q_min)

    def full(lanes, ones_row):
        y = [sbox(v + 1) for v in lanes]
        n0 = sum(y) if ones_row else red(sum(y))
        n = [n0, red(sum(y)), red(sum(y))]      # matrix entries < p
        see(*n)
        return n

    def permute(lanes):
        for f in range(4):
            lanes = full(lanes, f != 0)
        s0, s1, s2 = lanes
        for pair in range(29):
            second = pair < 28
            z0 = sbox(s0 + 1)
            n0 = red(z0 + s1 + s2)
            z1 = Fraction(0)
            if second:
                z1 = sbox(n0 + 1)
                n0 = red(z1 + s1 + s2 + z0)
            s2 = up(s2 + (z0 + z1) * rho + 1)           # REDC(s2 R + u z0 + u' z1), narrow digits
            s1 = s1 + z0 + z1                          # two lazy adds + normalize
            see(n0, s1, s2)
            if pair % 4 == 3:
                s1 = fold(s1)
                see(s1)
            s0 = n0
        lanes = [s0, s1, s2]
        for f in range(4):
            lanes = full(lanes, f != 0)
        return lanes

    entry = [Fraction(32), Fraction(16), Fraction(16)]
    out = permute(entry)
    assert out[0] < 32                          # the capacity lane enters the next permutation / canonicalize
    assert out[1] < 9 and out[2] < 9            # + an absorbed input or the padding 1: < 16p at the next entry
    assert fold(Fraction((1 << 261) - 1, P)) < Fraction(6, 5)   # the fold brings any valid s1 below 1.2p
    assert worst < 120                          # headroom to 2^261 = 169.4p
