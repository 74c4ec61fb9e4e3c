"""CPU: the partial rounds' Montgomery form dot4_add_uc (csrc/imt_mont_asm_rec.hpp, the C++ form mont_dot<4, true,
true> in the host build) bit for bit against a Python model at the corners of its operand domain: four constants and
four window values with limbs < 2^29 (up to 2^261 - 1), an addend with normalised limbs.  Also the compiled kernel of
the test-only harness tests/native/rec_form.hip: it runs the assembly, takes its constants from SGPRs, and reads no
lane.  The GPU twin is tests/test_gpu_rec_form.py."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "rec_form.hip")
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
NL, W = 9, 29
MASK, M32 = (1 << W) - 1, (1 << 32) - 1
PL = [(P >> (W * i)) & MASK for i in range(NL)]
N0INV32 = 0xEFFFFFFF                       # -p^-1 mod 2^32
assert (P * N0INV32 + 1) % (1 << 32) == 0


def limbs(x):
    return [(x >> (W * i)) & MASK for i in range(NL - 1)] + [x >> (W * (NL - 1))]


def value(l):
    return sum(v << (W * i) for i, v in enumerate(l))


def model(u, x, e):
    """dot4_add_uc column by column, as the generator lays it out: returns (r limbs, peak of the 64-bit accumulator)."""
    acc, peak, m, r = 0, 0, [0] * NL, [0] * NL
    for k in range(NL):
        for t in range(4):
            for i in range(k + 1):
                acc += u[t][i] * x[t][k - i]
        for i in range(k):
            acc += m[i] * PL[k - i]
        m[k] = ((acc & M32) * N0INV32) & M32
        acc += m[k] * PL[0]
        peak = max(peak, acc)
        acc >>= W
    for k in range(NL, 2 * NL - 1):
        for t in range(4):
            for i in range(k - (NL - 1), NL):
                acc += u[t][i] * x[t][k - i]
        for i in range(k - (NL - 1), NL):
            acc += m[i] * PL[k - i]
        acc += e[k - NL]
        peak = max(peak, acc)
        r[k - NL] = acc & MASK
        acc >>= W
    r[NL - 1] = (acc + e[NL - 1]) & M32
    return r, peak


def corpus(n_blocks=48, seed=0xD04A):
    """uniform constants per block of 64 lanes and per-lane window values / addends, drawn from the domain's corners"""
    rng = random.Random(seed)
    top = (1 << 261) - 1                                     # every limb 2^29 - 1
    corners = [0, 1, P - 1, top, MASK << (W * (NL - 1)), (1 << 232) - 1, P, 2 * P - 1]
    def draw():
        k = rng.randrange(4)
        if k == 0:
            return rng.choice(corners)
        if k == 1:
            return rng.randrange(P)
        if k == 2:
            return value([rng.choice([0, MASK, rng.randrange(1 << W)]) for _ in range(NL)])
        return rng.randrange(1 << 261)
    uni, lanes = [], []
    for b in range(n_blocks):
        if b == 0:
            uni.append([top] * 4)
        elif b == 1:
            uni.append([P - 1] * 4)
        else:
            uni.append([draw() for _ in range(4)])
        for j in range(64):
            if j == 0:
                lanes.append([top] * 5)                      # every limb at its bound: the column peak
            elif j == 1:
                lanes.append([0] * 5)
            else:
                lanes.append([draw() for _ in range(5)])
    to = lambda rows: np.array([[limbs(v) for v in row] for row in rows], dtype=np.uint32)
    return to(uni), to(lanes)


def expected(uni, lanes):
    out, peak = [], 0
    for j in range(lanes.shape[0]):
        u = [list(map(int, uni[j // 64][t])) for t in range(4)]
        x = [list(map(int, lanes[j][t])) for t in range(4)]
        e = list(map(int, lanes[j][4]))
        r, pk = model(u, x, e)
        peak = max(peak, pk)
        # what the form computes: r = (sum u x + m p) / R + e, so r = sum u x / R + e mod p, r < sum u x / R + e + 8p
        t = sum(value(a) * value(b) for a, b in zip(u, x))
        v = value(r)
        assert (v - value(e)) * (1 << 261) % P == t % P
        assert v < t / (1 << 261) + value(e) + 8 * P
        out.append(r)
    assert peak < 1 << 64                                    # the accumulator never carries out of bit 63
    return np.array(out, dtype=np.uint32), peak


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_dot4_add_uc_host_form_matches_model():
    so = os.path.join(ROOT, "tests", "native", "librecform_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(SRC), os.path.getmtime(
            os.path.join(CSRC, "imt_device.hpp"))):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-I", CSRC, "-o", so, SRC],
                       check=True)
    lib = ctypes.CDLL(so)
    uni, lanes = corpus()
    want, peak = expected(uni, lanes)
    assert peak > (1 << 64) * 7 // 10                         # all limbs at their bound: columns past 0.7 * 2^64
    out = np.zeros((lanes.shape[0], NL), np.uint32)
    lib.rec_form_host(_p(np.ascontiguousarray(lanes)), _p(np.ascontiguousarray(uni)), _p(out),
                      ctypes.c_uint(lanes.shape[0]))
    assert (out == want).all()


def test_dot4_add_uc_kernel_assembly(tmp_path):
    """the harness kernel holds the form's 413 v_mad_u64_u32 (324 limb products with the constant as an SGPR, 81 digit
    products, 8 addend limbs), no v_readfirstlane, and vector instructions only inside the form"""
    out = tmp_path / "rec_form.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC,
                    "--cuda-device-only", "-S", "-o", str(out), SRC], check=True, capture_output=True)
    asm = out.read_text()
    body = re.search(r"^rek_dot4_add_uc:[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M).group(1)
    assert body.count(";;#ASMSTART") == 1 and "v_readfirstlane" not in body
    form = body.split(";;#ASMSTART")[1].split(";;#ASMEND")[0]     # the inline-asm block (addressing mads are outside)
    assert all(l.strip().startswith("v_") for l in form.splitlines() if l.strip())
    mads = [l for l in form.splitlines() if "v_mad_u64_u32" in l]
    assert len(mads) == 324 + 81 + 8
    assert sum(l.split(",")[2].strip().startswith("s") for l in mads) == 324
