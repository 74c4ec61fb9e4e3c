"""Shared by the tests of the 1..16-input hash (test_hash_n_cpu.py, test_gpu_hash_n.py) and the generator of their golden
file: the row / cell formulas, the oracle's trace with buffers large enough for 16 inputs, a sponge restated over the
oracle's bare permutation, and the fixed input vectors.  TEST INFRASTRUCTURE ONLY."""
import ctypes

import numpy as np

import oracle_lib
from oracle_lib import P

MAX_INPUTS = 16
LENS = list(range(1, MAX_INPUTS + 1))
R256 = (1 << 256) % P
R261 = (1 << 261) % P
SCALE = {0: 1, 1: R256, 2: R261}          # what a stored value is multiplied by in format 0 / 1 / 2


def rows(length):
    """a permutation that absorbs k inputs assigns 3 + k + 600 new values"""
    return 605 * (length // 2) + 603 + (length & 1)


def cells(length):
    return 2256 * (length // 2) + 2250 + 3 * (length & 1)


def ints(a):
    return [int.from_bytes(x.tobytes(), "little") for x in np.asarray(a, np.uint8).reshape(-1, 32)]


def to_arr(xs, fmt=0):
    """ints -> uint8 [len(xs), 32] in format `fmt`"""
    return oracle_lib.ints_to_arr([x * SCALE[fmt] % P for x in xs])


def sponge(oracle, xs):
    """The absorb and padding rule written out over the oracle's bare permutation: state [2^64, 0, 0]; every full pair
    is added to lanes 1, 2 and permuted; then the leftover input (if any) and the padding 1 go into the next free
    lane(s) and the state is permuted once more; the result is lane 1."""
    s = [1 << 64, 0, 0]
    full = len(xs) // 2
    for c in range(full):
        s = oracle.permute([s[0], (s[1] + xs[2 * c]) % P, (s[2] + xs[2 * c + 1]) % P])
    if len(xs) & 1:
        s = oracle.permute([s[0], (s[1] + xs[-1]) % P, (s[2] + 1) % P])
    else:
        s = oracle.permute([s[0], (s[1] + 1) % P, s[2]])
    return s[1]


def oracle_trace(oracle, xs):
    """oracle_lib.Oracle.hash_trace with buffers sized for 16 inputs (its own 6000 cells hold up to 3)"""
    cap, wcap = cells(MAX_INPUTS) + 16, rows(MAX_INPUTS) + 16
    col = np.empty((cap, 32), np.uint8)
    desc = (oracle_lib.TraceCell * cap)()
    wit = np.empty((wcap, 32), np.uint8)
    nc, nw, row = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint32()
    rc = oracle.lib.orc_hash_trace(b"".join(oracle_lib.b32(x) for x in xs), len(xs), col.ctypes.data_as(ctypes.c_void_p), desc,
                                   ctypes.c_size_t(cap), ctypes.byref(nc), wit.ctypes.data_as(ctypes.c_void_p),
                                   ctypes.c_size_t(wcap), ctypes.byref(nw), ctypes.byref(row))
    assert rc == 0, rc
    d = np.frombuffer(bytes(desc), dtype=np.dtype([("kind", "u1"), ("gate", "u1"), ("region", "<u2"), ("index", "<u4")]))[:nc.value]
    return dict(cells=col[:nc.value].copy(), kind=d["kind"].copy(), gate=d["gate"].copy(), index=d["index"].copy(),
                region=d["region"].copy(), witness=wit[:nw.value].copy(), out_row=row.value)


def oracle_rows(oracle, xs):
    """the witness rows alone, uint8 [rows, 32] canonical"""
    wit = np.empty((rows(len(xs)), 32), np.uint8)
    nc, nw, row = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint32()
    rc = oracle.lib.orc_hash_trace(b"".join(oracle_lib.b32(x) for x in xs), len(xs), None, None, ctypes.c_size_t(0),
                                   ctypes.byref(nc), wit.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len(wit)),
                                   ctypes.byref(nw), ctypes.byref(row))
    assert rc == 0 and nw.value == len(wit) and row.value == len(wit) - 4, (rc, nw.value, row.value)
    return wit


def scaled(arr, fmt):
    """canonical uint8 [..., 32] -> the same values in format `fmt`"""
    if fmt == 0:
        return arr
    a = np.asarray(arr, np.uint8)
    return to_arr(ints(a), fmt).reshape(a.shape)


def golden_inputs(length):
    """the one fixed input vector per length of tests/golden/hash_n_digest.json"""
    return oracle_lib.synth_values(length, 0x494D5400 + length)


def vectors(length):
    """[0] * len, [p - 1] * len and three synthetic vectors"""
    return [[0] * length, [P - 1] * length] + [oracle_lib.synth_values(length, 0x484E0000 + 64 * k + length) for k in range(3)]
