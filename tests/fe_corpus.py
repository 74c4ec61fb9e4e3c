"""Operand corpus of the device Montgomery forms (tests/fe_model.py FORMS), one domain per form.

Each operand slot has a domain: a limb width (29 bits, or 30 where a lazy add feeds the form) and an exclusive value
bound taken from the callers' worst-case proofs, or "const" for a wave-uniform table constant (< p).  Per form the
corpus holds, at the corners of the domain: zero, all limbs at the maximum width (the top limb as large as the bound
allows), k p - 1, k p, k p + 1 up to the bound, 2^261 - 1 where the bound allows it, the real Poseidon tables as
constants, operands from a seeded search that maximises the model's column peak, and 2^16 random rows.

Rows are [n, slots, 9] uint64 (fe_model.operands order).  Uniform slots are constant over each aligned block of
BLOCK rows, because the GPU harness reads them per block, as the real kernels read them per round.
"""
import random

import numpy as np

import fe_model as fm
from fe_model import NL, P, W

BLOCK = 64
N_RANDOM = 1 << 16

# the callers' value bounds, in units of p (proofs: tests/test_rescaled_schedule.py::test_rescaled_schedule_bounds,
# tests/test_fe_forms.py::test_coop_schedule_bounds / test_trace_schedule_bounds)
THREAD = 120 * P        # every operand of permute()
COOP = 60 * P           # every operand of coop::permute (entry lanes < 32p)
TRACE = 4 * P           # every operand of permute_trace
CONST = "const"

# slot domains in fe_model.operands order: (limb width, bound) or CONST
DOMAINS = {
    # permute(): sbox mont_mul(x, x4, x) -- x4 a product, x = lane + constant (lazy); load_fe / store_fe: raw < 2^256
    "mul_vv": [(29, THREAD), (30, THREAD)],
    "sqr_v": [(30, THREAD)],                                    # the S-box input x = lane + constant, then x^2
    "dot3_uc": [CONST, (29, THREAD)] * 3,                       # rows of sc_mats / sc_row times the lanes
    "dot4_uc": [CONST, (29, THREAD)] * 4,                       # sc_row[p + 1], sc_gamma[p + 1] times v0, s1, s2, z0
    "dot2_add_uc_narrow": [CONST, (29, THREAD)] * 2 + [(29, THREAD)],   # sc_u z0 + sc_u' z1 + s2 R
    # t_sqr (< 4p) and the coop S-box (v = S + k, lazy)
    "sqr_v_narrow": [(30, COOP)],
    "mul_vv_adds_narrow": [(29, TRACE), (29, TRACE), CONST],    # t_mul_add(x, x, x4, c)
    "mul_uc_narrow": [CONST, (29, TRACE)],                      # t_mulc(row[0], s0)
    "mul_uc_add_narrow": [CONST, (29, TRACE), (29, TRACE)],     # t_mulc_add(row[i], s_i, acc)
    "redc_v_narrow": [(29, TRACE)],                             # t_emit, canonical output
    # coop: x^2 with both operands x = S + k (lazy), col x, x4 x, row s
    "mul_vv_narrow": [(30, COOP), (30, COOP)],
    "mul_vv_add_narrow": [(29, COOP), (29, COOP), (30, 2 * COOP)],    # x4 (row0 x | col x) + (U1 + U2 | S)
    "dot3_vv_narrow": [(29, COOP)] * 6,                         # M rows (table entries, per lane) times Y
}
# which real tables feed the constant slots (PoseidonConsts / TraceConsts member names)
TABLES = {
    "dot3_uc": ["sc_mats", "sc_row"],
    "dot4_uc": ["sc_row4"],
    "dot2_add_uc_narrow": ["sc_u"],
    "mul_vv_adds_narrow": ["t.full_c", "t.partial"],
    "mul_uc_narrow": ["t.mats", "t.row"],
    "mul_uc_add_narrow": ["t.mats", "t.row", "t.col_hat"],
    "dot3_vv_narrow": ["mats", "sp_row"],       # per lane in the coop schedule
}

# ---- the constant tables, parsed from the raw struct images -----------------------------------------------------------
RP, RF = 57, 8
PC_LAYOUT = [("rc_full", (RF, 3)), ("rc_h2p2", (3,)), ("k_partial", (RP,)), ("mats", (2, 3, 3)), ("sp_row", (RP, 3)),
             ("sp_col", (RP, 2)), ("cap0", ()), ("one", ()), ("from_canon", ()), ("from_mont256", ()),
             ("to_mont256", ()), ("int_one", ()), ("zero_leaf", ()), ("sc_rc", (RF, 3)), ("sc_mats", (RF, 3, 3)),
             ("sc_k", (RP,)), ("sc_row", (RP, 3)), ("sc_gamma", (RP,)), ("sc_u", (RP,))]
TC_LAYOUT = [("absorb", (3, 3)), ("full_c", (RF, 3)), ("partial", (RP,)), ("mats", (2, 3, 3)), ("row", (RP, 3)),
             ("col_hat", (RP, 2))]


def parse(words, layout):
    out, off = {}, 0
    for name, shape in layout:
        cnt = int(np.prod(shape)) if shape else 1
        a = np.asarray(words[off:off + cnt * NL], np.uint64).reshape(shape + (NL,))
        out[name] = a
        off += cnt * NL
    assert off == len(words), (off, len(words))
    return out


def table_sets(name, pc, tc):
    """the real constant sets of a form's uniform slots: a list of [n_const_slots, 9] arrays"""
    sets = []
    for t in TABLES.get(name, []):
        if t == "sc_mats":
            for f in range(RF):
                for row in range(3):
                    if row == 0 and f not in (0, RF // 2):
                        continue            # row (1, 1, 1) is a plain sum there
                    sets.append(pc["sc_mats"][f, row])
        elif t == "sc_row":
            sets += [pc["sc_row"][p] for p in range(RP)]
        elif t == "sc_row4":
            sets += [np.concatenate([pc["sc_row"][p + 1], pc["sc_gamma"][p + 1][None]]) for p in range(0, RP - 1, 2)]
        elif t == "sc_u":
            sets += [np.stack([pc["sc_u"][p], pc["sc_u"][min(p + 1, RP - 1)]]) for p in range(0, RP, 2)]
        elif t == "t.full_c":
            sets += [tc["full_c"][f, i][None] for f in range(RF) for i in range(3)]
        elif t == "t.partial":
            sets += [tc["partial"][p][None] for p in range(RP)]
        elif t == "t.mats":
            sets += [tc["mats"][k, r, c][None] for k in range(2) for r in range(3) for c in range(3)]
        elif t == "t.row":
            sets += [tc["row"][p, c][None] for p in range(RP) for c in range(3)]
        elif t == "t.col_hat":
            sets += [tc["col_hat"][p, c][None] for p in range(RP) for c in range(2)]
        elif t == "mats":
            sets += [pc["mats"][k, r] for k in range(2) for r in range(3)]
        elif t == "sp_row":
            sets += [pc["sp_row"][p] for p in range(RP)]
    return sets


# ---- corners --------------------------------------------------------------------------------------------------------
def _max_top(low, bound, width):
    return min((1 << width) - 1, (bound - 1 - low) >> (W * (NL - 1)))


def max_limbs(width, bound):
    """all limbs at the maximum width, the top limb as large as the bound allows"""
    low = [(1 << width) - 1] * (NL - 1)
    return low + [_max_top(fm.from_limbs(low), bound, width)]


def denormalise(x, width):
    """the same value with its low limbs widened to `width` bits where a borrow from the next limb allows"""
    l = fm.to_limbs(x)
    if width == W:
        return None
    for i in range(NL - 2, -1, -1):
        if l[i + 1] > 0 and l[i] + (1 << W) < 1 << width:
            l[i + 1] -= 1
            l[i] += 1 << W
    return l if l != fm.to_limbs(x) else None


def corners(dom):
    if dom == CONST:
        return [fm.to_limbs(0), fm.to_limbs(1), fm.to_limbs(P - 1), max_limbs(W, P)]
    width, bound = dom
    vals = {0, 1, bound - 1}
    for k in range(1, bound // P + 1):
        vals |= {x for x in (k * P - 1, k * P, k * P + 1) if x < bound}
    if bound > (1 << 261) - 1:
        vals.add((1 << 261) - 1)
    out = [fm.to_limbs(v) for v in sorted(vals)]
    out += [d for d in (denormalise(v, width) for v in sorted(vals)) if d is not None]
    out.append(max_limbs(width, bound))
    return out


def random_limbs(rng, dom, n):
    """n random operands of a domain: eight limbs uniform over the width, the top limb uniform below what the bound
    leaves for any low part; a quarter with every low limb at the maximum"""
    if dom == CONST:
        x = [rng.randrange(P) for _ in range(n)]
        return np.array([fm.to_limbs(v) for v in x], np.uint64)
    width, bound = dom
    g = np.random.default_rng(rng.randrange(1 << 32))
    low = g.integers(0, 1 << width, size=(n, NL - 1), dtype=np.uint64)
    low[: n // 4] = (1 << width) - 1
    top_cap = max(0, (bound >> (W * (NL - 1))) - 2)      # low < 2^(29*8 + 1): top * 2^232 + low < bound
    top = g.integers(0, top_cap + 1, size=(n, 1), dtype=np.uint64)
    top[: n // 8] = top_cap
    return np.concatenate([low, top], axis=1)


def _clamp(row, doms):
    for s, dom in enumerate(doms):
        if dom == CONST:
            continue
        width, bound = dom
        low = fm.from_limbs(row[s][:NL - 1])
        row[s][NL - 1] = min(row[s][NL - 1], _max_top(low, bound, width))
    return row


def peak_search(name, rng, uniform_sets, generations=40, pop=4 * BLOCK):
    """seeded hill climb on the model's column peak: keep the best quarter, mutate limbs to their maximum or to a
    random value, inside the slot domains.  Constant slots stay at the given set (one per block)."""
    doms = DOMAINS[name]
    lane = [s for s, d in enumerate(doms) if d != CONST]
    cidx = {s: k for k, s in enumerate(s for s, d in enumerate(doms) if d == CONST)}
    best = []
    for u in uniform_sets:
        rows = []
        for _ in range(pop):
            r = [list(map(int, u[cidx[s]])) if d == CONST else None for s, d in enumerate(doms)]
            for s in lane:
                w, b = doms[s]
                r[s] = max_limbs(w, b) if rng.random() < 0.5 else [rng.randrange(1 << w) for _ in range(NL)]
            rows.append(_clamp(r, doms))
        for _ in range(generations):
            peak = model(name, np.array(rows, np.uint64))[1]
            order = np.argsort(-peak.astype(np.float64), kind="stable")
            keep = [rows[i] for i in order[: pop // 4]]
            rows = list(keep)
            while len(rows) < pop:
                r = [list(x) for x in rng.choice(keep)]
                for _ in range(rng.randrange(1, 4)):
                    s = rng.choice(lane)
                    i = rng.randrange(NL)
                    w = doms[s][0]
                    r[s][i] = (1 << w) - 1 if rng.random() < 0.6 else rng.randrange(1 << w)
                rows.append(_clamp(r, doms))
        best += rows[:BLOCK]
    return best


# ---- model on corpus rows -------------------------------------------------------------------------------------------
def split(name, X):
    """[n, slots, 9] -> the arguments of fe_model.mont"""
    f = fm.FORMS[name]
    if len(fm.operands(name)) == 1:
        return (X[:, 0],)
    nt = f.nt
    a = np.stack([X[:, 2 * t] for t in range(nt)])
    b = np.stack([X[:, 2 * t + 1] for t in range(nt)])
    return (a, b, X[:, 2 * nt]) if f.add else (a, b)


def model(name, X):
    return fm.mont(name, *split(name, X))


def build(name, pc, tc, seed=0xFE):
    """the corpus of one form: [n, slots, 9] uint64, uniform slots constant per aligned block of BLOCK rows"""
    rng = random.Random(seed * 1000 + sorted(fm.FORMS).index(name))
    doms = DOMAINS[name]
    cslots = [s for s, d in enumerate(doms) if d == CONST]
    lslots = [s for s, d in enumerate(doms) if d != CONST]
    csets = [np.array([corners(CONST)[i]] * len(cslots), np.uint64) for i in range(4)]
    tsets = [np.asarray(t, np.uint64).reshape(-1, NL) for t in table_sets(name, pc, tc)]
    if cslots:
        tsets = [t for t in tsets if t.shape[0] == len(cslots)]
    # corner rows of the lane slots: each slot runs through its corners while the others rotate through theirs
    cl = [corners(doms[s]) for s in lslots]
    n = max(len(c) for c in cl)
    lane_rows = []
    for shift in (0, 1, 7, 31):
        for i in range(n):
            lane_rows.append([cl[j][(i + shift * j) % len(cl[j])] for j in range(len(lslots))])
    for j in range(len(lslots)):                 # every slot at its largest value against every corner of the others
        for i in range(n):
            lane_rows.append([cl[k][-1] if k == j else cl[k][i % len(cl[k])] for k in range(len(lslots))])
    if not cslots:                               # per-lane table entries stand in for the lane slots they feed
        for t in tsets:
            for c in corners(doms[lslots[0]]):
                row = [list(map(int, t[(s // 2) % t.shape[0]])) if s % 2 == 0 else c for s in range(len(lslots))]
                lane_rows.append(row)
    lane_rows = np.array(lane_rows, np.uint64)
    uni = csets + tsets if cslots else [np.zeros((0, NL), np.uint64)]

    blocks = []

    def emit(lanes, u):
        X = np.zeros((lanes.shape[0], len(doms), NL), np.uint64)
        X[:, lslots] = lanes
        if cslots:
            X[:, cslots] = u[None]
        blocks.append(X)

    # corner lanes against every constant set, a block at a time
    for b0 in range(0, lane_rows.shape[0], BLOCK):
        for u in (uni if cslots else uni[:1]):
            emit(lane_rows[b0:b0 + BLOCK], u)
            if not cslots:
                break
    # the peak search, against the constant set with the widest limbs
    best = peak_search(name, rng, [csets[3]] if cslots else [np.zeros((0, NL), np.uint64)])
    best = np.array(best, np.uint64)
    for b0 in range(0, best.shape[0], BLOCK):
        emit(best[b0:b0 + BLOCK][:, lslots], csets[3] if cslots else None)
    # random rows, constants from the tables and from random values
    rnd = np.stack([random_limbs(rng, doms[s], N_RANDOM + 37) for s in lslots], axis=1)
    for b0 in range(0, rnd.shape[0], BLOCK):
        u = None
        if cslots:
            u = rng.choice(tsets) if tsets and rng.random() < 0.7 else random_limbs(rng, CONST, len(cslots))
        emit(rnd[b0:b0 + BLOCK], u)
    # every block is full except the last one of the corpus: ragged at the end of the last wave
    full = [np.resize(b, (BLOCK,) + b.shape[1:]) for b in blocks[:-1]]       # short blocks repeat their rows
    return np.concatenate(full + [blocks[-1]])


# ---- the helpers: inputs at the corners of what their callers hand them ---------------------------------------------
def _values(bound, rng, extra=(), n=4096):
    vals = {0, 1, bound - 1} | set(extra)
    for k in range(1, bound // P + 1):
        vals |= {x for x in (k * P - 1, k * P, k * P + 1) if x < bound}
    vals = sorted(vals) + [rng.randrange(bound) for _ in range(n)]
    return np.array([fm.to_limbs(v) for v in vals], np.uint64)


def _words(vals):
    return np.array([[(v >> (32 * i)) & fm.M32 for i in range(8)] for v in vals], np.uint64)


def helper_inputs(name, rng):
    """(in_words, out_words, inputs [n, in_words]) of one helper kernel"""
    if name == "canonicalize":                        # normalised, < 32p (the exit lanes of permute)
        return 9, 9, _values(32 * P, rng)
    if name == "fold_p":                              # normalised, < 2^261 (lane s1 of permute)
        return 9, 9, np.concatenate([_values(1 << 261, rng, extra=[(1 << 261) - 1, 120 * P]),
                                     np.array([max_limbs(W, 1 << 261)], np.uint64)])
    if name == "normalize":                           # lazy sums of up to three normalised values: 31-bit limbs
        x = random_limbs(rng, (31, 3 * 120 * P), 4096)
        return 9, 9, np.concatenate([x, np.array([max_limbs(31, 3 * 120 * P), max_limbs(30, 2 * 120 * P)], np.uint64)])
    if name.startswith("cond_sub_p_shl") or name.startswith("csub"):
        sh = int(name[-1])
        around = [(P << sh) + d for d in range(-3, 4)]
        bound = 32 * P if name.startswith("cond") else 6 * P
        return 9, 9, _values(bound, rng, extra=[v for v in around if 0 <= v < bound])
    if name == "t_add":                               # a < 3.2p, b < p
        a = _values(16 * P // 5, rng)
        b = _values(P, rng, n=a.shape[0])[: a.shape[0]]
        b = np.resize(b, a.shape)
        return 18, 9, np.concatenate([a, np.roll(b, 3, axis=0)], axis=1)
    if name == "pack":                                # normalised, < 2^256
        return 9, 8, _values(1 << 256, rng, extra=[(1 << 256) - 1, 5 * P])
    if name == "unpack" or name.startswith("load_fe"):   # any eight words
        vals = [0, 1, P - 1, P, P + 1, (1 << 256) - 1, (1 << 254), 5 * P] + [rng.randrange(1 << 256) for _ in range(4096)]
        vals += [rng.randrange(P) for _ in range(1024)]
        return 8, (10 if name.startswith("load") else 9), _words(vals)
    if name.startswith("store_fe"):                   # device form: canonical for FMT_DEVICE, else < 32p
        return 9, 8, _values(P if name.endswith("2") else 32 * P, rng)
    if name == "store_mont256":                       # normalised, < 4p
        top_eq = [fm.from_limbs([0] * 8 + [fm._top_limb_of_multiple(k)]) + d for k in (1, 2, 3) for d in (0, 1 << 200)]
        return 9, 8, _values(4 * P, rng, extra=[v for v in top_eq if v < 4 * P])
    raise KeyError(name)


HELPERS = ["canonicalize", "fold_p", "normalize"] + ["cond_sub_p_shl%d" % s for s in range(5)] + ["csub0", "csub1",
           "t_add", "pack", "unpack", "load_fe0", "load_fe1", "load_fe2", "store_fe0", "store_fe1", "store_fe2",
           "store_mont256"]


def helper_model(name, X, consts):
    if name == "canonicalize":
        return fm.canonicalize(X)
    if name == "fold_p":
        return fm.fold_p(X)
    if name == "normalize":
        return fm.normalize(X)
    if name.startswith("cond_sub_p_shl"):
        return fm.cond_sub_p_shl(X, int(name[-1]))
    if name.startswith("csub"):
        return fm.csub(X, int(name[-1]))
    if name == "t_add":
        return fm.t_add(X[:, :9], X[:, 9:])
    if name == "pack":
        return fm.pack(X)
    if name == "unpack":
        return fm.unpack(X)
    if name.startswith("load_fe"):
        r, ok = fm.load_fe(X, int(name[-1]), consts)
        return np.concatenate([r, ok[:, None].astype(np.uint64)], axis=1)
    if name.startswith("store_fe"):
        return fm.store_fe(X, int(name[-1]), consts)
    if name == "store_mont256":
        return fm.store_mont256(X)
    raise KeyError(name)


_CACHE = {}


def corpus(name, pc, tc):
    if name not in _CACHE:
        _CACHE[name] = build(name, pc, tc)
    return _CACHE[name]


def consts_of(pc):
    return {k: [int(x) for x in pc[k]] for k in ("from_canon", "from_mont256", "int_one", "to_mont256")}
