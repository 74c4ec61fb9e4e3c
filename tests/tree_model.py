"""The sorted list of an indexed tree as plain Python, and the step scripts played on it (TEST INFRASTRUCTURE ONLY).

TreeModel is the specification of the list imt_itree keeps: Python integers, a list in insertion order, a sorted list
beside it.  Its rules are written from include/imt.h and the reference's update_idx_leaf, not from the library's own
restatements (imt_prep_logic.hpp, imt_filter_logic.hpp, host_filter).  It knows nothing of hashes: roots, proofs and
witness rows of a state come from the CPU oracle, which is loaded with the model's preimages (oracle_root,
oracle_proofs, oracle_rows; cached per state).

scripts() returns the committed step scripts of tests/test_gpu_tree_sequences.py: sequences of the twelve ways into the
tree and of refused calls, generated coverage-directed from the literal seeds below so that every ordered pair of
writer kinds is adjacent somewhere with a light check between the two and somewhere with a full one
(tests/test_tree_model.py asserts that).  The first nine scripts are the first pass: the ten older kinds on every shape,
byte for byte what they were before the mixed batch existed (their digest is asserted).  A second pass with seeds of its
own appends scripts on the plain shapes (the mixed batch refuses placed and partitioned trees) for exactly the pairs in
which a mixed batch takes part.  The writer kinds:
   1 insert_batch, host pointers, GPU prepare        6 apply_batch, GPU prepare
   2 insert_batch, IMT_HOST_PREP                     7 apply_batch, IMT_HOST_PREP
   3 insert_batch, device pointers + IMT_PIPELINE,   8 apply_filtered, prepare mode alternating
     left in flight                                  9 rewind(s)
   4 insert_filtered, GPU prepare                   10 load of a snapshot taken from the model
   5 insert_filtered, IMT_HOST_PREP                 11 a refused call of one of the other kinds
  12 mixed_batch with INSERTs and READs, host and   13 mixed_batch of READs only, a writer that must change nothing;
     device pointers in turn, the sibling layout       host and device pointers in turn
     changing at half that rate

A third pass (THIRD_SEEDS, _ThirdGenerator; the first two passes are frozen by digest) plays the seven ways into the tree
merged since, on MemberModel, every pair of them adjacent at both check levels and every pair with an older kind at some:
  14 insert_bulk, host / device pointers, both layouts    18 mixed_pipelined / apply_mixed_pipelined, left in flight
  15 apply_pipelined, left in flight, root_out on the     19 load_values, host / device, the three formats; a prefix of
     device; IMT_HOST_PREP and IMT_INPUTS_READY in turn       an earlier state or unrelated values
  16 mixed_filtered, host / device, layouts, MEMBERs      20 reserve: grow, shrink to the smallest legal capacity, the same
  17 apply_mixed / apply_mixed_filtered, MEMBERs
Kinds 14, 16, 17 and 18 are IMT_ERR_ARG on placed and partitioned trees and appear there as refusals only.  A step of
the third pass may carry the check level NO_CHECK: the next step follows with no call in between, so that writers enter
with several pipelined batches (kinds 3, 15, 18) still in flight.

view_schedule() and view_rounds() say which views (imt_itree_view_*) tests/test_gpu_view_sequences.py keeps alive beside a
script, what each answers after every step and when its cache must be rebuilt; the scripts themselves do not change.
"""
import bisect
import random
from collections import namedtuple

import numpy as np

import insert_corpus as ic
import oracle_lib
from oracle_lib import P, ints_to_arr

NEW, ZERO, PRESENT, REPEATED, FOREIGN = 0, 1, 2, 3, 4        # IMT_VAL_*
NONE = (1 << 64) - 1
LIGHT, FULL = "light", "full"
NO_CHECK = "none"                    # the third check level: the next step follows with no call in between (third pass only)
KINDS = tuple(range(1, 11))          # the ten older writer kinds: what the first pass of scripts() plays
REFUSED = 11
MIXED, MIXED_READS = 12, 13
ALL_KINDS = KINDS + (MIXED, MIXED_READS)
BULK, APPLY_PIPE, MIXED_FILT, APPLY_MIXED, MIXED_PIPE, LOAD_VALUES, RESERVE = NEW_KINDS = tuple(range(14, 21))
KINDS19 = ALL_KINDS + NEW_KINDS      # what the third pass of scripts() plays
PIPELINED = (3, APPLY_PIPE, MIXED_PIPE)                 # left in flight until the next check or a synchronous call's own wait
PLAIN_ONLY = (MIXED, MIXED_READS, BULK, MIXED_FILT, APPLY_MIXED, MIXED_PIPE)     # IMT_ERR_ARG on placed and partitioned trees
OP_INSERT, OP_READ = 0, 1            # IMT_OP_*
OP_MEMBER = 2                        # under IMT_MEMBER_OPS
NEW_REFUSALS = ("bulk_stored", "bulk_repeat", "bulk_zero", "bulk_full", "bulk_ge_p", "pipe_stored", "pipe_full", "lv_zero",
                "lv_repeat", "lv_ge_p", "lv_full", "reserve_below", "reserve_npot", "reserve_above", "member_absent",
                "op2_no_flag", "plain_only")
REFUSALS = ("stored", "repeat", "zero", "full", "ge_p", "broken_link", "rewind_past")
REFUSAL_CODE = dict(stored="VALUE", repeat="VALUE", zero="VALUE", full="FULL", ge_p="NONCANONICAL", broken_link="VALUE",
                    rewind_past="RANGE", mixed_read_stored="VALUE", mixed_read_inserted_earlier="VALUE",
                    mixed_insert_repeat="VALUE", mixed_full="FULL", mixed_ge_p="NONCANONICAL",
                    bulk_stored="VALUE", bulk_repeat="VALUE", bulk_zero="VALUE", bulk_full="FULL", bulk_ge_p="NONCANONICAL",
                    pipe_stored="VALUE", pipe_full="FULL", lv_zero="VALUE", lv_repeat="VALUE", lv_ge_p="NONCANONICAL",
                    lv_full="FULL", reserve_below="RANGE", reserve_npot="RANGE", reserve_above="RANGE",
                    member_absent="VALUE", op2_no_flag="ARG", plain_only="ARG")
MIXED_REFUSALS = ("mixed_read_stored", "mixed_read_inserted_earlier", "mixed_insert_repeat", "mixed_full", "mixed_ge_p")
REWIND_VARIANTS = ("interior", "size-1", "noop", "one")
REWIND_ORDER = ("interior", "size-1", "interior", "noop", "interior", "one")
SIZE_LIMIT = 150                     # no script grows a tree past this many leaves
TOPS = (0x1234_5678_9ABC_DEF0, 0x2FFF_0000_0000_0001)      # top 64 bits shared by groups of values (both below p's)


class Refused(Exception):
    """the call is refused with IMT_ERR_<code> and changes nothing; bad_op: *bad_op of a mixed batch refused for a value"""

    def __init__(self, code, bad_op=None):
        super().__init__(code)
        self.code, self.bad_op = code, bad_op

    bad_pos = property(lambda self: self.bad_op)       # of imt_itree_load_values


class TreeModel:
    """vals[i] = the value of leaf i (vals[0] = 0, the sentinel); indices that leave the model are global."""

    def __init__(self, depth, cap, index_base=0, part_mod=0, part_res=0):
        self.depth, self.cap, self.index_base, self.part_mod, self.part_res = depth, cap, index_base, part_mod, part_res
        self._reset([0])

    def _reset(self, vals):
        self.vals = list(vals)
        self.where = {v: i for i, v in enumerate(self.vals)}
        self.order = sorted(self.vals)

    @property
    def size(self):
        return len(self.vals)

    def mine(self, v):
        return self.part_mod <= 1 or v % self.part_mod == self.part_res

    def _append(self, v):
        pos = bisect.bisect_left(self.order, v)
        low_val = self.order[pos - 1]                      # pos >= 1: the sentinel is stored and v > 0
        succ = self.order[pos] if pos < len(self.order) else None
        row = dict(low=self.index_base + self.where[low_val], largest=int(succ is None),
                   low_leaf=(low_val, succ or 0, self.index_base + self.where[succ] if succ is not None else 0))
        self.order.insert(pos, v)
        self.where[v] = len(self.vals)
        self.vals.append(v)
        return row

    # ---- writers ----
    def insert(self, vals):
        """imt_itree_insert_batch / _apply_batch: all or nothing.  Returns per insertion the low leaf's index, its
        preimage before the insertion and is_largest."""
        vals = list(vals)
        if self.size + len(vals) > self.cap:
            raise Refused("FULL")
        if any(v >= P for v in vals):
            raise Refused("NONCANONICAL")
        if len(set(vals)) != len(vals) or any(v == 0 or v in self.where or not self.mine(v) for v in vals):
            raise Refused("VALUE")
        return [self._append(v) for v in vals]

    def classify(self, vals):
        """(status, leaf_index, accepted values) of imt_itree_insert_filtered, nothing changed.  The first that applies:
        ZERO, FOREIGN, PRESENT, REPEATED, NEW."""
        if any(v >= P for v in vals):
            raise Refused("NONCANONICAL")
        status, leaf, acc, first = [], [], [], {}
        for v in vals:
            if v == 0:
                s, l = ZERO, self.index_base
            elif not self.mine(v):
                s, l = FOREIGN, NONE
            elif v in self.where:
                s, l = PRESENT, self.index_base + self.where[v]
            elif v in first:
                s, l = REPEATED, first[v]
            else:
                s, l = NEW, self.index_base + self.size + len(acc)
                first[v] = l
                acc.append(v)
            status.append(s)
            leaf.append(l)
        if self.size + len(acc) > self.cap:
            raise Refused("FULL")
        return status, leaf, acc

    def filtered(self, vals):
        status, leaf, acc = self.classify(list(vals))
        self.insert(acc)
        return status, leaf, acc

    def mixed(self, vals, ops):
        """imt_itree_mixed_batch, from include/imt.h (DEFINED BY THE SEQUENCE ALONE): walk the operations in order, an
        INSERT is insert() of the one value, a READ is nm_witness() of it against the list at that moment.  Returns
        (the values inserted, [(position, low index, low-leaf preimage, is_largest, INSERTs before it)] of the READs).
        Refused as insert_batch refuses -- FULL counts the INSERTs only -- or with VALUE and the smallest offending
        position: an INSERT insert() refuses there, a READ of 0, of a stored value or of one inserted earlier in the
        batch.  A refusal leaves the model as it was."""
        vals, ops = list(vals), list(ops)
        if self.index_base or self.part_mod > 1:
            raise Refused("ARG")
        if self.size + ops.count(OP_INSERT) > self.cap:
            raise Refused("FULL")
        if any(v >= P for v in vals):
            raise Refused("NONCANONICAL")
        start, acc, reads = self.size, [], []
        try:
            for p, (v, op) in enumerate(zip(vals, ops)):
                if op == OP_INSERT:
                    self.insert([v])
                    acc.append(v)
                else:
                    reads.append((p, ) + self.nm_witness(v) + (len(acc), ))
        except Refused:
            self.rewind(start)
            raise Refused("VALUE", p)
        return acc, reads

    def rewind(self, s):
        if s == 0 or s > self.size:
            raise Refused("RANGE")
        self._reset(self.vals[:s])

    def load(self, preimages):
        """preimages: [(val, next_val, next_idx)] in leaf order.  One sorted chain from the sentinel or nothing."""
        pre = [tuple(p) for p in preimages]
        n = len(pre)
        if n == 0:
            raise Refused("ARG")
        if n > self.cap:
            raise Refused("FULL")
        if any(x >= P for p in pre for x in p):
            raise Refused("NONCANONICAL")
        vals = [p[0] for p in pre]
        if vals[0] != 0 or len(set(vals)) != n or not all(self.mine(v) for v in vals[1:]):
            raise Refused("VALUE")
        chain = sorted(range(n), key=vals.__getitem__)
        for i, j in zip(chain, chain[1:]):
            if pre[i][1:] != (vals[j], self.index_base + j):
                raise Refused("VALUE")
        if pre[chain[-1]][1:] != (0, 0):
            raise Refused("VALUE")
        self._reset(vals)

    def reserve(self, new_cap):
        """imt_itree_reserve: another capacity, nothing else.  RANGE unless new_cap is a power of two in [2, 2^31], at most
        2^depth and at least the size."""
        if not 2 <= new_cap <= 1 << 31 or new_cap & (new_cap - 1) or new_cap > 1 << self.depth or new_cap < self.size:
            raise Refused("RANGE")
        self.cap = new_cap

    def load_values(self, vals):
        """imt_itree_load_values: the model a fresh one becomes after insert(vals).  ARG for no values, FULL, then
        NONCANONICAL before VALUE (a 0, a repeat, a foreign residue), both with bad_pos = the smallest position that is
        >= p, 0, foreign or equal to a value at a smaller position (it rides in Refused.bad_op)."""
        vals = list(vals)
        if not vals:
            raise Refused("ARG")
        if len(vals) + 1 > self.cap:
            raise Refused("FULL")
        seen, bad = set(), []
        for p, v in enumerate(vals):
            if v >= P or v == 0 or not self.mine(v) or v in seen:
                bad.append(p)
            seen.add(v)
        if bad:
            raise Refused("NONCANONICAL" if any(v >= P for v in vals) else "VALUE", bad[0])
        self._reset([0] + vals)

    # ---- readers ----
    def preimages(self, indices):
        """{val, next_val, next_idx} of local leaves `indices`: next_idx global, all zero at and beyond size"""
        out = []
        for i in indices:
            if i >= self.size:
                out.append((0, 0, 0))
                continue
            pos = bisect.bisect_right(self.order, self.vals[i])
            succ = self.order[pos] if pos < len(self.order) else None
            out.append((self.vals[i], succ or 0, self.index_base + self.where[succ] if succ is not None else 0))
        return out

    def find_low(self, v):
        if v >= P:
            raise Refused("NONCANONICAL")
        if v == 0 or v in self.where or not self.mine(v):
            raise Refused("VALUE")
        return self.index_base + self.where[self.order[bisect.bisect_left(self.order, v) - 1]]

    def lookup(self, v):
        if v >= P:
            raise Refused("NONCANONICAL")
        if v == 0:
            return ZERO, self.index_base
        if not self.mine(v):
            return FOREIGN, NONE
        if v in self.where:
            return PRESENT, self.index_base + self.where[v]
        return NEW, self.find_low(v)

    def nm_witness(self, v):
        low = self.find_low(v)
        leaf = self.preimages([low - self.index_base])[0]
        return low, leaf, int(leaf[1] == 0)

    def probes(self):
        """the fixed probe set of a state: absent values of this tree's residue -- neighbours of stored values, 1,
        p - 1, values that share their top 64 bits with a stored one or with each other"""
        step = max(1, self.part_mod)
        stored = self.vals[1:]
        pick = stored[:6] + stored[-6:] + [self.order[-1], self.order[len(self.order) // 2]]
        cand = [1, P - 1, step, P - step]
        for v in pick:
            cand += [v - step, v + step, v ^ (1 << 130), (v >> 192 << 192) | 7, (v >> 192 << 192) | (v & 0xFFFF) << 64]
        cand += [(TOPS[0] << 192) + k for k in range(1, 7)]
        out = []
        for v in cand:
            if 0 < v < P and self.mine(v) and v not in self.where and v not in out:
                out.append(v)
        return out


# ---------------------------------------------------------------- shapes, steps, scripts
Shape = namedtuple("Shape", "name depth cap placement partition")
Step = namedtuple("Step", "kind refusal vals arg check")
Script = namedtuple("Script", "name shape steps")
_G5 = ic.BY_NAME["placed_g5"]
SHAPES = (
    Shape("d3", 3, 8, None, (0, 0)),
    Shape("d8", 8, 64, None, (0, 0)),
    Shape("d32", 32, 256, None, (0, 0)),
    Shape("placed_g5", _G5.depth, _G5.cap, tuple(_G5.placement), (0, 0)),
    Shape("part3", 16, 128, None, (3, 1)),
)
SEEDS = (0x54530001, 0x54530002, 0x54530003, 0x54530004, 0x54530005, 0x54530006, 0x54530007, 0x54530008, 0x54530009,
         0x5453000A, 0x5453000B, 0x5453000C, 0x5453000D, 0x5453000E, 0x5453000F, 0x54530010, 0x54530011, 0x54530012,
         0x54530013, 0x54530014, 0x54530015, 0x54530016, 0x54530017, 0x54530018, 0x54530019, 0x5453001A, 0x5453001B,
         0x5453001C, 0x5453001D, 0x5453001E, 0x5453001F, 0x54530020)
SCRIPT_STEPS = 30


def index_base(shape):
    return shape.placement[1] << shape.depth if shape.placement else 0


def new_model(shape, vals=None):
    from member_model import MemberModel       # TreeModel with IMT_OP_MEMBER and the filtered twins; it imports this module
    m = MemberModel(shape.depth, shape.cap, index_base(shape), *shape.partition)
    if vals is not None:
        m._reset(vals)
    return m


def writer_kind(step):
    return REFUSED if step.refusal else step.kind


def play(m, step):
    """One step on model m.  Accepted: dict(acc=the values inserted, status, leaf, reads) (what applies; reads: the READ
    rows of a mixed batch as TreeModel.mixed returns them).  A refused step raises Refused and leaves m as it was."""
    k = step.kind
    if k in (1, 2, 3, 6, 7):
        m.insert(step.vals)
        return dict(acc=list(step.vals))
    if k in (4, 5, 8):
        status, leaf, acc = m.filtered(step.vals)
        return dict(acc=acc, status=status, leaf=leaf)
    if k == 9:
        m.rewind(step.arg)
        return {}
    if k in (MIXED, MIXED_READS):
        acc, reads = m.mixed(step.vals, step.arg["ops"])
        return dict(acc=acc, reads=reads)
    if k == BULK:                                              # the tree of insert_batch; refused where a mixed batch is
        if m.index_base or m.part_mod > 1:
            raise Refused("ARG")
        m.insert(step.vals)
        return dict(acc=list(step.vals))
    if k == APPLY_PIPE:
        m.insert(step.vals)
        return dict(acc=list(step.vals))
    if k in (MIXED_FILT, APPLY_MIXED, MIXED_PIPE):
        ops, members = step.arg["ops"], step.arg["members"]
        if k == MIXED_FILT or (k == APPLY_MIXED and step.arg["filtered"]):
            if m.index_base or m.part_mod > 1 or any(op > (OP_MEMBER if members else OP_READ) for op in ops):
                raise Refused("ARG")
            status, leaf, carried, (acc, reads) = m.mixed_filtered(step.vals, ops)
            return dict(acc=acc, reads=reads, status=status, leaf=leaf, carried=carried)
        acc, reads = m.mixed(step.vals, ops, members)
        return dict(acc=acc, reads=reads, carried=list(range(len(ops))))
    if k == LOAD_VALUES:
        m.load_values(step.arg["vals"])
        return {}
    if k == RESERVE:
        m.reserve(step.arg)
        return {}
    m.load(step.arg["pre"])
    return {}


def trace(script):
    """[(step, vals before, vals after, outcome or the Refused raised)] of a script on a fresh model"""
    m, out = new_model(script.shape), []
    for st in script.steps:
        before = tuple(m.vals)
        try:
            res = play(m, st)
        except Refused as e:
            res = e
        out.append((st, before, tuple(m.vals), res))
    return out


# ---------------------------------------------------------------- views beside a script
# What tests/test_gpu_view_sequences.py keeps alive while it plays a script, and what every view must then answer.  A view
# at size s of a tree that holds `vals` is a model reset to vals[:s]; while len(vals) < s it answers nothing (IMT_ERR_RANGE).
HEAD, BEHIND, SMALLER = "at the head", "behind the head", "tree smaller than the view"
MAX_VIEWS = 4                        # live at once, the one at size 1 included
VIEW_EVERY = 4                       # a new view after every accepted step whose index is a multiple of this
REPLAY_MAX = 16                      # insertions replayed per view and round
VIEW_ROUNDS_OTHER_FORMS = 2          # the scripts replayed on the thread and quad forms: a round after every second step
ViewRound = namedtuple("ViewRound", "size state prefix build since n_replay")


def changes_content(st, before, after, res):
    """Does the step change the tree's contents as include/imt.h counts them (A VIEW FOLLOWS THE TREE): an insertion of
    any kind that accepted something (a mixed batch with an INSERT among them), a load, a rewind below the current size.
    A refused call, a filtered batch that accepted nothing, a mixed batch of READs only and a rewind to the current size
    do not."""
    if isinstance(res, Refused) or st.kind == RESERVE:         # another capacity is no other content
        return False
    if st.kind <= 8 or st.kind in (MIXED, MIXED_READS, BULK, APPLY_PIPE, MIXED_FILT, APPLY_MIXED, MIXED_PIPE):
        return bool(res["acc"])                                # a block of READs / MEMBERs only, or nothing carried out: no change
    return st.arg < len(before) if st.kind == 9 else True      # load and load_values: always


def view_schedule(script):
    """[(sizes closed, sizes created)] per step, both after the step and before its round of queries; the view at size 1
    exists before step 0 and is never closed.  Views are told apart by their size: there is at most one of a size.  After
    every accepted step whose index is a multiple of VIEW_EVERY a view is created unless one of its size exists: at the
    size M the tree then has and below it, at 1 + (M - 1) // 2, in turn.  With MAX_VIEWS alive the oldest one that is not
    the view at size 1 is closed first."""
    live, out, made = [1], [], 0
    for i, (st, before, after, res) in enumerate(trace(script)):
        closed, created = (), ()
        if i % VIEW_EVERY == 0 and not isinstance(res, Refused) and st.check != NO_CHECK:      # NO_CHECK: not one call
            M = len(after)
            s = M if made % 2 == 0 else 1 + (M - 1) // 2
            if s not in live:
                made += 1
                if len(live) == MAX_VIEWS:
                    closed = (live.pop(1), )
                live.append(s)
                created = (s, )
        out.append((closed, created))
    return out


def view_rounds(script, every=1):
    """Per step the round of queries that follows it: [ViewRound] of the live views, oldest first; with every = 2 only the
    steps of even index are followed by a round ([] for the others: what they changed shows in the next round).
         state      HEAD, BEHIND or SMALLER
         prefix     the values the view answers for (vals[:size] of the tree after the step); None while SMALLER
         build      the round rebuilds the view's cache (imt_itree_view_stats' count goes up by one): its first answered
                    round, and every answered round with a content-changing step since the last answered one
         since      the writer kinds of those content-changing steps, oldest first
         n_replay   min(insertions that follow the view's size, REPLAY_MAX)"""
    stale, since, out = {1: True}, {1: ()}, []
    for i, ((st, before, after, res), (closed, created)) in enumerate(zip(trace(script), view_schedule(script))):
        if changes_content(st, before, after, res):
            for s in stale:
                stale[s], since[s] = True, since[s] + (writer_kind(st), )
        for s in closed:
            del stale[s], since[s]
        for s in created:
            stale[s], since[s] = True, ()
        M, rnd = len(after), []
        for s in stale if i % every == 0 and st.check != NO_CHECK else ():       # no round behind a NO_CHECK step either
            if M < s:                                             # answers nothing, builds nothing, stays as stale as it is
                rnd.append(ViewRound(s, SMALLER, None, False, since[s], 0))
                continue
            rnd.append(ViewRound(s, HEAD if s == M else BEHIND, after[:s], stale[s], since[s], min(M - s, REPLAY_MAX)))
            stale[s], since[s] = False, ()
        out.append(rnd)
    return out


class _Generator:
    """Chooses every next writer kind among those that still have an uncovered pair behind the step before."""

    def __init__(self):
        self.need = {(a, b, lv) for a in KINDS for b in KINDS for lv in (LIGHT, FULL)}
        self.need11 = set(KINDS)
        self.refusals = list(REFUSALS)
        self.n_rewind = self.n_load = self.n_refused = self.n_apply_filtered = 0
        self.d3_full = self.d3_room_again = False

    def done(self):
        return not (self.need or self.need11 or self.refusals)

    # -- values --
    def fresh(self, k, exclude=()):
        m, rng, out = self.m, self.rng, []
        step = max(1, m.part_mod)
        while len(out) < k:
            r = rng.random()
            if self.specials:
                v = self.specials.pop()
            elif r < 0.25 and m.size > 1:
                v = rng.choice(m.vals[1:]) + rng.choice((-step, step))
            elif r < 0.45:
                v = (rng.choice(TOPS) << 192) | rng.getrandbits(192)
            else:
                v = self.pool.pop()
            if 0 < v < P and m.mine(v) and v not in m.where and v not in out and v not in exclude:
                out.append(v)
        return out

    def mixed(self, room):
        m, rng = self.m, self.rng
        n, out, n_new = rng.randint(1, 16), [], 0
        for i in range(n):
            r = rng.random()
            if (r < 0.55 or (i == 0 and room)) and n_new < room:
                out += self.fresh(1, out)
                n_new += 1
            elif r < 0.67:
                out.append(0)
            elif r < 0.82 and m.size > 1:
                out.append(rng.choice(m.vals[1:]))
            elif r < 0.94 and out:
                out.append(rng.choice(out))
            elif m.part_mod > 1:
                w = rng.choice(m.vals[1:] + [4])
                out.append(w + 1 if w + 1 < P else w - 2)             # another subtree's residue
            else:
                out.append(0)
        return out

    # -- what can follow --
    def room(self):
        return min(self.m.cap, SIZE_LIMIT) - self.m.size

    def feasible(self, k):
        return self.room() >= 1 if k in (1, 2, 3, 6, 7) else True

    def refusal_feasible(self, name):
        m, room = self.m, self.m.cap - self.m.size
        if name in ("zero", "ge_p"):
            return room >= 1
        if name == "stored":
            return room >= 1 and m.size > 1
        if name == "repeat":
            return room >= 2
        if name == "full":
            return room + 1 <= 16
        if name == "broken_link":
            return m.size >= 2
        return True

    def out_degree(self, k, levels=(LIGHT, FULL)):
        return sum((k, b, lv) in self.need for b in KINDS for lv in levels)

    def choose(self, prev, pos):
        """(kind, refusal name or None) of the next step"""
        rng = self.rng
        d3 = self.shape.cap == 8
        if d3 and self.m.size == self.m.cap and not self.d3_full and not (prev and prev.refusal):
            self.d3_full = True
            return None, "full"
        if d3 and self.d3_full and not self.d3_room_again and self.m.size == self.m.cap:
            self.d3_room_again = True
            return 9, None
        feas = [k for k in KINDS if self.feasible(k)]
        if prev is None:
            cands = []
        elif prev.refusal:
            cands = [k for k in feas if k in self.need11]
        else:
            cands = [k for k in feas if (prev.kind, k, prev.check) in self.need]
        # once per script a refused call right behind a host-prepared batch: the device index is stale when it arrives
        stale = prev is not None and not prev.refusal and prev.kind in (2, 5, 7) and not self.stale_refusal and pos >= 3
        if stale:
            self.stale_refusal = True
        if prev is not None and not prev.refusal and (stale or ((self.refusals or self.need11) and (not cands or pos % 9 == 5))):
            names = [r for r in self.refusals if self.refusal_feasible(r)] or \
                    [r for r in REFUSALS[self.n_refused % 7:] + REFUSALS[:self.n_refused % 7] if self.refusal_feasible(r)]
            self.host_side = stale
            return None, names[0]
        pool = cands or ([9, 10] if self.room() == 0 else feas)      # nothing uncovered from here: at least make room
        best = max(self.out_degree(k) for k in pool)
        return rng.choice([k for k in pool if self.out_degree(k) == best]), None

    def level(self, k):
        a, b = self.out_degree(k, (LIGHT,)), self.out_degree(k, (FULL,))
        return LIGHT if a > b else FULL if b > a else self.rng.choice((LIGHT, FULL))

    def refusal_level(self):
        return (LIGHT, FULL)[self.n_refused & 1]

    # -- the steps --
    def snapshot_of(self, vals):
        return tuple(new_model(self.shape, vals).preimages(range(len(vals))))

    def make_rewind(self):
        m = self.m
        for _ in range(len(REWIND_ORDER)):
            v = "interior" if self.shape.cap == 8 and m.size == m.cap else REWIND_ORDER[self.n_rewind % len(REWIND_ORDER)]
            self.n_rewind += 1
            if v == "interior" and m.size >= 4:
                return self.rng.randint(2, m.size - 2)
            if v == "size-1" and m.size >= 2:
                return m.size - 1
            if v == "noop":
                return m.size
            if v == "one" and m.size >= 2:
                return 1
        return m.size

    def make_load(self):
        m, rng, c = self.m, self.rng, self.n_load
        self.n_load += 1
        source, longer = ("earlier", "unrelated")[(c >> 1) & 1], bool((c >> 2) & 1)
        fits = (lambda n: n > m.size) if longer else (lambda n: n < m.size)
        vals = None
        if source == "earlier":
            states = [s for s in self.history if fits(len(s)) and list(s) != m.vals]
            if states:
                vals = list(rng.choice(states))
        if vals is None:
            source = "unrelated"
            lo, hi = (m.size + 1, min(m.cap, SIZE_LIMIT, m.size + 24)) if longer else (1, m.size - 1)
            if lo > hi:
                lo, hi = 1, min(m.cap, 12)
            n = rng.randint(lo, hi)
            vals = [0] + [self.other.pop() for _ in range(n - 1)]
        return dict(pre=self.snapshot_of(vals), device=bool(c & 1), fmt=c % 3, source=source)

    def make_refusal(self, name):
        m, rng, c = self.m, self.rng, self.n_refused
        self.n_refused += 1
        room = m.cap - m.size
        if name == "rewind_past":
            return Step(9, name, None, m.size + 1, None)
        if name == "broken_link":
            pre = [list(p) for p in self.snapshot_of(m.vals)]
            pre[rng.randrange(m.size)][2] += 1
            return Step(10, name, None, dict(pre=tuple(tuple(p) for p in pre), device=bool(c & 1), fmt=0, source="broken"), None)
        if name == "full":
            kinds = (2, 5, 7) if self.host_side else (1, 4, 6, 2, 5, 7, 8)
            return Step(kinds[c % len(kinds)], name, tuple(self.fresh(room + 1)), c % 2 == 0, None)
        k = min(rng.randint(2, 5), room)
        good = self.fresh(k - 1)
        if name == "ge_p":
            kinds = (5, 7, 2) if self.host_side else (4, 1, 7, 5, 6, 8, 2)
            return Step(kinds[c % len(kinds)], name, tuple(good + [P + rng.randrange(3)]), c % 2 == 0, None)
        bad = dict(stored=lambda: rng.choice(m.vals[1:]), repeat=lambda: rng.choice(good), zero=lambda: 0)[name]()
        vals = good + [bad]
        rng.shuffle(vals)
        return Step(((2, 7) if self.host_side else (1, 2, 6, 7))[c % (2 if self.host_side else 4)], name, tuple(vals), None, None)

    def make(self, kind, refusal):
        if refusal:
            return self.make_refusal(refusal)
        if kind in (1, 2, 3, 6, 7):
            return Step(kind, None, tuple(self.fresh(self.rng.randint(1, min(16, self.room())))), None, None)
        if kind in (4, 5, 8):
            arg = None
            if kind == 8:
                arg = bool(self.n_apply_filtered & 1)        # IMT_HOST_PREP on every other call
                self.n_apply_filtered += 1
            return Step(kind, None, tuple(self.mixed(self.room())), arg, None)
        if kind == 9:
            return Step(9, None, None, self.make_rewind(), None)
        return Step(10, None, None, self.make_load(), None)

    def script(self, number, shape, seed):
        self.shape, self.rng, self.m = shape, random.Random(seed), new_model(shape)
        own = lambda s, n: [v for v in oracle_lib.synth_values(n, s) if self.m.mine(v)]
        self.pool, self.other = own(seed, 1500), own(seed ^ 0x00FF0000, 2400)
        self.specials = [v for v in (P - 1, 1) if self.m.mine(v)]
        self.history = [tuple(self.m.vals)]
        self.stale_refusal = self.host_side = False
        steps, prev = [], None
        while len(steps) < SCRIPT_STEPS and not (self.done() and len(steps) >= 8):
            kind, refusal = self.choose(prev, len(steps))
            st = self.make(kind, refusal)
            if st.refusal:
                check = self.refusal_level()
                self.refusals = [r for r in self.refusals if r != st.refusal]
            else:
                check = self.level(st.kind)
                if prev is not None and prev.refusal:
                    self.need11.discard(st.kind)
                elif prev is not None:
                    self.need.discard((prev.kind, st.kind, prev.check))
                play(self.m, st)
                self.history.append(tuple(self.m.vals))
            st = st._replace(check=check)
            steps.append(st)
            prev = st
        steps[-1] = steps[-1]._replace(check=FULL)
        return Script(f"{shape.name}_{number:02d}", shape, tuple(steps))


MIXED_SHAPES = SHAPES[:3]            # d3, d8, d32: imt_itree_mixed_batch refuses placed and partitioned trees
MIXED_SEEDS = (0x4D530001, 0x4D530002, 0x4D530003, 0x4D530004, 0x4D530005, 0x4D530006, 0x4D530007, 0x4D530008, 0x4D530009,
               0x4D53000A, 0x4D53000B, 0x4D53000C)
MIXED_MAX_OPS = {3: 16, 8: 16, 32: 12}     # operations per mixed batch at a depth: every READ is an oracle proof of that depth


class _MixedGenerator(_Generator):
    """The second pass: the (a, b, level) triples in which a or b is a mixed batch (kinds 12 and 13), both of them right
    after a refused call, the refusals of the mixed batch.  A generator of its own, with seeds of its own, so that the
    scripts of the first pass stay what they are."""

    def __init__(self):
        super().__init__()
        new = (MIXED, MIXED_READS)
        self.need = {(a, b, lv) for a in ALL_KINDS for b in ALL_KINDS for lv in (LIGHT, FULL) if a in new or b in new}
        self.need11 = set(new)
        self.refusals = list(MIXED_REFUSALS)
        self.n_mixed = {MIXED: 0, MIXED_READS: 0}
        self.n_mixed_refused = 0
        self.d3_reads_full = False
        self.n_behind_stale = 0
        self.stories = ["is_largest flips", "low leaf moves", "more operations than room"]

    def done(self):
        return not (self.need or self.need11 or self.refusals or self.stories) and self.d3_reads_full

    def out_degree(self, k, levels=(LIGHT, FULL)):
        return sum((k, b, lv) in self.need for b in ALL_KINDS for lv in levels)

    def refusal_level(self):
        return LIGHT if self.host_side else super().refusal_level()   # no reader between the refusal and the mixed batch

    def fresh(self, k, exclude=()):
        self.specials = []                                 # 1 and p - 1 are asked for by READs here (read_value)
        return super().fresh(k, exclude)

    def feasible(self, k):
        return self.room() >= 1 if k in (1, 2, 3, 6, 7, MIXED) else True

    def refusal_feasible(self, name):
        m, room = self.m, self.m.cap - self.m.size
        if name == "mixed_read_stored":
            return m.size > 1
        if name == "mixed_read_inserted_earlier":
            return room >= 1
        if name == "mixed_insert_repeat":
            return room >= 2
        if name == "mixed_full":
            return room + 1 <= 8
        if name == "mixed_ge_p":
            return True
        return super().refusal_feasible(name)

    def choose(self, prev, pos):
        rng, m = self.rng, self.m
        d3, after_refusal = self.shape.cap == 8, prev is not None and bool(prev.refusal)
        if d3 and m.size == m.cap and not after_refusal:
            if not self.d3_reads_full:                     # READs only on a full tree: legal
                self.d3_reads_full = True
                return MIXED_READS, None
            if "mixed_full" in self.refusals:
                self.host_side = False
                return None, "mixed_full"
        feas = [k for k in ALL_KINDS if self.feasible(k)]
        if prev is None:
            cands = []
        elif after_refusal:
            cands = [k for k in feas if k in self.need11]
        else:
            cands = [k for k in feas if (prev.kind, k, prev.check) in self.need]
        # once per script a refused host-prepared call right behind a host-prepared batch, a mixed batch behind it: the
        # device index that the mixed batch needs is stale through both
        stale = prev is not None and not after_refusal and prev.kind in (2, 5, 7) and prev.check == LIGHT and \
            not self.stale_refusal and pos >= 3 and self.room() >= 2
        if stale:
            self.stale_refusal = True
            self.host_side = True
            names = [r for r in ("ge_p", "stored", "full") if self.refusal_feasible(r)]
            return None, names[self.n_refused % len(names)]
        if prev is not None and not after_refusal and (self.refusals or self.need11) and (not cands or pos % 6 == 4):
            names = [r for r in self.refusals if self.refusal_feasible(r)] or \
                    [r for r in MIXED_REFUSALS[self.n_mixed_refused % 5:] + MIXED_REFUSALS[:self.n_mixed_refused % 5]
                     if self.refusal_feasible(r)]
            self.host_side = False
            return None, names[0]
        if after_refusal and prev.kind in (2, 5, 7):       # behind the refused host-prepared call: kind 12 and 13 in turn
            cands = [k for k in ((MIXED, MIXED_READS), (MIXED_READS, MIXED))[self.n_behind_stale & 1] if k in feas][:1]
            self.n_behind_stale += 1
        if after_refusal and not cands:                    # nothing owed behind a refusal: on to a mixed batch
            cands = [k for k in (MIXED, MIXED_READS) if k in feas]
        pool = cands or ([9, 10] if self.room() == 0 else feas)
        best = max(self.out_degree(k) for k in pool)
        return rng.choice([k for k in pool if self.out_degree(k) == best]), None

    # -- the values of the READs --
    def read_value(self, inserted, later, read):
        """a value a READ may ask for: not 0, below p, neither stored nor among `inserted` (the batch's INSERTs so far)"""
        m, rng = self.m, self.rng
        known = m.vals[1:] + inserted
        while True:
            r = rng.random()
            if r < 0.2 and later:
                v = rng.choice(later)                      # a later INSERT of this batch inserts it
            elif r < 0.35 and read:
                v = rng.choice(read)                       # already read in this batch
            elif r < 0.6 and known:
                v = rng.choice(known) + rng.choice((-1, 1))
            elif r < 0.8 and known:
                v = (rng.choice(known) >> 192 << 192) | rng.getrandbits(192)       # shares its top 64 bits with a stored one
            elif r < 0.85:
                v = rng.choice((1, P - 1))
            else:
                v = self.pool.pop()
            if 0 < v < P and v not in m.where and v not in inserted:
                return v

    def make_ops(self, kind, n_ins, n):
        """(vals, ops) of an accepted mixed batch of n operations, n_ins of them INSERTs"""
        m, rng = self.m, self.rng
        new = self.fresh(n_ins)
        ops = [OP_INSERT] * n_ins + [OP_READ] * (n - n_ins)
        rng.shuffle(ops)
        vals, inserted, read, later = [], [], [], list(new)
        for op in ops:
            if op == OP_INSERT:
                v = later.pop(0)
                inserted.append(v)
            else:
                v = self.read_value(inserted, later, read)
                read.append(v)
            vals.append(v)
        return vals, ops

    def story(self, name, room):
        """(vals, ops) of a kind-12 batch written for one of the cases tests/test_tree_model.py asks for, or None"""
        m, rng = self.m, self.rng
        top = m.order[-1]
        if name == "is_largest flips" and top + 4 < P and room >= 2:
            x = top + 2                                    # above every stored value: the READ's low leaf is the largest one
            return [x, x + 2, x, x - 1, x + 1, x + 1], [OP_READ, OP_INSERT, OP_READ, OP_READ, OP_READ, OP_INSERT]
        if name == "low leaf moves" and room >= 3:
            x, y = self.fresh(2)
            if x - 2 > 0 and x - 1 not in m.where and x - 2 not in m.where and y not in (x - 1, x - 2):
                return [x, x - 2, x, x - 1, y, x, y], [OP_READ, OP_INSERT, OP_READ, OP_INSERT, OP_READ, OP_READ, OP_INSERT]
        left = m.cap - m.size                              # FULL counts the INSERTs only: n > room >= INSERTs is accepted
        if name == "more operations than room" and 1 <= left < MIXED_MAX_OPS[self.shape.depth]:
            return self.make_ops(MIXED, rng.randint(1, min(left, 3)), rng.randint(left + 1, MIXED_MAX_OPS[self.shape.depth]))
        return None

    def mixed_arg(self, kind, ops):
        c = self.n_mixed[kind]
        self.n_mixed[kind] += 1
        return dict(ops=tuple(ops), device=bool(c & 1), item_major=bool((c >> 1) & 1))

    def make(self, kind, refusal):
        if kind not in (MIXED, MIXED_READS) or refusal:
            return super().make(kind, refusal)
        rng, room, top = self.rng, self.room(), MIXED_MAX_OPS[self.shape.depth]
        if kind == MIXED_READS:
            vals, ops = self.make_ops(kind, 0, rng.randint(1, top))
        else:
            got = None
            for name in list(self.stories):
                got = self.story(name, room)
                if got:
                    self.stories.remove(name)
                    break
            if not got:
                n = rng.randint(2, top)
                got = self.make_ops(kind, rng.randint(1, min(room, n - 1, 8)), n)
            vals, ops = got
        return Step(kind, None, tuple(vals), self.mixed_arg(kind, ops), None)

    def make_refusal(self, name):
        if name not in MIXED_REFUSALS:
            return super().make_refusal(name)
        m, rng = self.m, self.rng
        self.n_refused += 1
        self.n_mixed_refused += 1
        room = m.cap - m.size
        if name == "mixed_full":
            n_ins = room + 1
        elif name == "mixed_insert_repeat":
            n_ins = rng.randint(1, min(room - 1, 4))       # the repeated INSERT still fits: the refusal is VALUE, not FULL
        elif name == "mixed_read_inserted_earlier":
            n_ins = rng.randint(1, min(room, 4))
        else:
            n_ins = rng.randint(0, min(room, 4))
        vals, ops = self.make_ops(MIXED, n_ins, n_ins + rng.randint(1, 4))
        ins_at = [p for p, op in enumerate(ops) if op == OP_INSERT]
        if name == "mixed_read_stored":
            at, bad = rng.randint(0, len(ops)), (OP_READ, rng.choice(m.vals[1:]))
        elif name == "mixed_ge_p":
            at, bad = rng.randint(0, len(ops)), (OP_READ, P + rng.randrange(3))
        elif name == "mixed_full":
            at, bad = None, None
        else:
            src = rng.choice(ins_at)
            at = rng.randint(src + 1, len(ops))
            bad = (OP_READ if name == "mixed_read_inserted_earlier" else OP_INSERT, vals[src])
        if bad:
            ops.insert(at, bad[0])
            vals.insert(at, bad[1])
        kind = MIXED if OP_INSERT in ops else MIXED_READS
        c = self.n_mixed_refused
        return Step(kind, name, tuple(vals), dict(ops=tuple(ops), device=bool(c & 1), item_major=bool((c >> 1) & 1)), None)


THIRD_SHAPES = (Shape("d3", 3, 2, None, (0, 0)), Shape("d8", 8, 16, None, (0, 0)), Shape("d32", 32, 64, None, (0, 0)),
                SHAPES[3], SHAPES[4])          # the plain shapes start below their capacity: reserve has room to grow them
THIRD_ORDER = (1, 2, 0, 3, 4, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0)      # the shape of every script, into THIRD_SHAPES
THIRD_SEEDS = (0x54500001, 0x54500002, 0x54500003, 0x54500004, 0x54500005, 0x54500006, 0x54500007, 0x54500008, 0x54500009,
               0x5450000A, 0x5450000B, 0x5450000C, 0x5450000D, 0x5450000E, 0x5450000F, 0x54500010, 0x54500011, 0x54500012,
               0x54500013, 0x54500014)
THIRD_STEPS = 40
MAX_CAP = 256                        # no reserve of the scripts grows a tree past this capacity
RUN_KINDS = ((3, APPLY_PIPE, MIXED_PIPE, APPLY_PIPE, MIXED_PIPE, 3, APPLY_PIPE), (3, APPLY_PIPE, 3, APPLY_PIPE, APPLY_PIPE, 3, APPLY_PIPE))
STATE_STORIES = ("bulk, device index stale", "refused bulk, device index stale", "load_values, device index stale",
                 "reserve, mirror valid, device index stale", "reserve, mirror stale, device index valid",
                 "reserve, both valid", "MEMBERs behind a refused host-prepared call")


class _ThirdGenerator(_MixedGenerator):
    """The third pass: the seven kinds merged since the mixed batch (14 to 20).  Every ordered pair of them at both check
    levels, every pair of one of them and an older kind at some level, each right after a refused call, their refusals;
    and what no check between two steps makes possible: batches of several pipelined kinds in flight when the next writer
    enters, runs of pipelined steps long enough for the back-pressure of the fifth.  Seeds and scripts of its own."""

    def __init__(self):
        super().__init__()
        new = NEW_KINDS
        self.need = {(a, b, lv) for a in new for b in new for lv in (LIGHT, FULL)}
        self.need_any = {(a, b) for a in KINDS19 for b in KINDS19 if (a in new) != (b in new)}
        self.need11 = set(new)
        self.refusals = list(NEW_REFUSALS)
        self.stories, self.d3_reads_full = [], True
        self.n_new = dict.fromkeys(new, 0)
        self.need_flight = set(KINDS19)      # kinds that have yet to enter behind two batches in flight of two kinds
        self.n_runs, self.run_refusals = 0, 0
        self.d3_grown = False                # FULL, then reserve, then the same batch accepted
        self.state_stories = list(STATE_STORIES)
        self.n_flight_story = 0

    def done(self):
        return not (self.need or self.need_any or self.need11 or self.refusals or self.need_flight or self.state_stories) \
            and self.n_runs >= 2 and self.run_refusals >= 1 and self.d3_grown

    def left(self):
        return dict(pairs=sorted(self.need), pairs_any=sorted(self.need_any), after_refusal=sorted(self.need11), refusals=self.refusals,
                    flight=sorted(self.need_flight), states=self.state_stories, runs=self.n_runs, d3_grown=self.d3_grown)

    # -- what can follow --
    def feasible(self, k):
        if k in PLAIN_ONLY and not self.plain:
            return False
        return self.room() >= 1 if k in (1, 2, 3, 6, 7, MIXED, BULK, APPLY_PIPE) else True

    def refusal_feasible(self, name):
        m, room = self.m, self.m.cap - self.m.size
        if name not in NEW_REFUSALS:
            return super().refusal_feasible(name)
        if name in ("member_absent", "op2_no_flag") or name.startswith("bulk"):
            if not self.plain:
                return False
        if name == "plain_only":
            return not self.plain
        if name in ("bulk_stored", "pipe_stored"):
            return room >= 1 and m.size > 1
        if name == "bulk_repeat":
            return room >= 2
        if name in ("bulk_zero", "bulk_ge_p"):
            return room >= 1
        if name in ("bulk_full", "pipe_full"):
            return room + 1 <= 16
        if name == "lv_full":
            return m.cap <= 32
        if name == "lv_repeat":
            return m.cap >= 4
        if name == "reserve_below":
            return m.size >= 3
        if name == "reserve_npot":
            return self.npot() <= 1 << m.depth
        if name == "reserve_above":
            return m.depth <= 30
        return True

    def npot(self):
        v = 3
        while v < self.m.size:
            v *= 2
        return v

    def owed(self, a, b, lv):
        return (a, b, lv) in self.need or (a, b) in self.need_any

    def out_degree(self, k, levels=(LIGHT, FULL)):
        return sum(self.owed(k, b, lv) for b in KINDS19 if self.feasible(b) for lv in levels)

    def level(self, k):
        a, b = (sum((k, x, lv) in self.need for x in NEW_KINDS) for lv in (LIGHT, FULL))
        return LIGHT if a > b else FULL if b > a else self.rng.choice((LIGHT, FULL))

    def choose(self, prev, pos):
        rng = self.rng
        after_refusal = prev is not None and bool(prev.refusal)
        feas = [k for k in KINDS19 if self.feasible(k)]
        if self.room() < 4 and not after_refusal and prev is not None and prev.kind not in (9, RESERVE):
            grows = self.m.cap * 2 <= min(1 << self.m.depth, MAX_CAP)          # make room first: reserve where it can grow
            return (RESERVE if grows else 9), None
        if prev is None:
            cands = []
        elif after_refusal:
            cands = [k for k in feas if k in self.need11]
        else:
            lv = prev.check
            cands = [k for k in feas if self.owed(prev.kind, k, lv)]
        if prev is not None and not after_refusal and (self.refusals or self.need11) and (not cands or pos % 5 == 3):
            names = [r for r in self.refusals if self.refusal_feasible(r)] or \
                    [r for r in NEW_REFUSALS[self.n_refused % 17:] + NEW_REFUSALS[:self.n_refused % 17] if self.refusal_feasible(r)]
            return None, names[0]
        pool = cands or feas
        best = max(self.out_degree(k) for k in pool)
        if best == 0 and not cands and not after_refusal:      # nothing owed can follow from here
            if self.room() < 16 and self.m.size > 8:
                return 9, None                                 # what is owed may need room
            return None, None                                  # this shape has given what it can: the script ends
        return rng.choice([k for k in pool if self.out_degree(k) == best]), None

    # -- the stories: steps in a fixed order, for what the pair coverage does not bring about --
    def plan(self, prev, pos):
        m, rng, left, room = self.m, self.rng, THIRD_STEPS - pos, self.room()
        if prev is not None and prev.refusal:
            return []
        d3 = self.shape.depth == 3
        if d3 and not self.d3_grown and m.cap < 8 and m.cap - m.size + 1 <= 8 and left >= 4:
            self.d3_grown = True
            kind, name = ((BULK, "bulk_full"), (APPLY_PIPE, "pipe_full"))[self.n_refused & 1]
            vals = tuple(self.fresh(m.cap - m.size + 1))
            return [dict(refusal=name, vals=vals), dict(kind=RESERVE, grow=True), dict(kind=kind, vals=vals)]
        if not d3 and pos in (1, 2) and m.cap < 64:            # room for the runs and the stories below
            return [dict(kind=RESERVE, grow=True)]
        if not d3 and self.n_runs < 2 and pos >= 4 and left >= 11 and room >= 16 and m.size > 1:
            kinds = RUN_KINDS[0 if self.plain else 1]
            run = [dict(kind=k, small=True, check=NO_CHECK, host_prep=(i == 3)) for i, k in enumerate(kinds)]
            del run[-1]["check"]
            bad = dict(refusal="member_absent", kind=MIXED_PIPE, check=NO_CHECK) if self.plain and self.n_runs else \
                dict(refusal="pipe_stored", check=NO_CHECK)
            run.insert(4, bad)
            self.n_runs += 1
            self.run_refusals += 1
            return run
        if pos % 5 == 1 and pos >= 3 and left >= 5 and room >= 6:
            todo = sorted(k for k in self.need_flight if k not in PIPELINED and self.feasible(k))
            if todo:
                pipes = [k for k in PIPELINED if self.feasible(k)]
                c = self.n_flight_story
                self.n_flight_story += 1
                a, b = pipes[c % len(pipes)], pipes[(c + 1) % len(pipes)]
                new = [k for k in todo if k in NEW_KINDS]
                return [dict(kind=a, small=True, check=NO_CHECK), dict(kind=b, small=True, check=NO_CHECK), dict(kind=(new or todo)[0])]
        if pos % 5 == 0 and pos >= 5 and left >= 5 and room >= 8 and m.size > 2:
            for name in self.state_stories:
                i = STATE_STORIES.index(name)
                if i in (0, 1, 6) and not self.plain:
                    continue
                self.state_stories.remove(name)
                host = dict(kind=(2, 7)[pos & 1], check=LIGHT)
                self.host_side = True
                return [[host, dict(kind=BULK)], [host, dict(refusal="bulk_stored")], [host, dict(kind=LOAD_VALUES)],
                        [host, dict(kind=RESERVE)], [dict(kind=6, check=LIGHT), dict(kind=RESERVE)],
                        [dict(kind=2, check=FULL), dict(kind=RESERVE)],
                        [host, dict(refusal="stored", check=LIGHT), dict(kind=(MIXED_FILT, APPLY_MIXED, MIXED_PIPE)[pos % 3], members=True)]][i]
        return []

    # -- the steps --
    def make_block(self, n_ins, n, members, noisy, top):
        """(vals, ops) of a block the unfiltered calls accept: n_ins INSERTs of fresh values, READs of absent ones and,
        with members, MEMBERs of values stored or inserted earlier in the block.  noisy: up to three operations more that
        a filtered twin skips -- a 0, a stored value, a value an earlier INSERT of the block put in, a MEMBER of an absent one."""
        m, rng = self.m, self.rng
        new = self.fresh(n_ins)
        ops = [OP_INSERT] * n_ins + [rng.choice((OP_READ, OP_MEMBER)) if members else OP_READ for _ in range(n - n_ins)]
        rng.shuffle(ops)
        vals, inserted, read, later = [], [], [], list(new)
        for i, op in enumerate(ops):
            there = m.vals[1:] + inserted
            if op == OP_INSERT:
                v = later.pop(0)
                inserted.append(v)
            elif op == OP_MEMBER and there:
                v = rng.choice(there)
            else:
                ops[i] = OP_READ
                v = self.read_value(inserted, later, read)
                read.append(v)
            vals.append(v)
        for _ in range(rng.randint(1, 3) if noisy else 0):
            if len(vals) >= top:
                break
            at, r = rng.randint(0, len(vals)), rng.random()
            earlier = [v for v, o in zip(vals[:at], ops[:at]) if o == OP_INSERT]
            any_op = rng.choice((OP_INSERT, OP_READ, OP_MEMBER) if members else (OP_INSERT, OP_READ))
            if r < 0.3:
                bad = (any_op, 0)
            elif r < 0.6 and m.size > 1:
                bad = (rng.choice((OP_INSERT, OP_READ)), rng.choice(m.vals[1:]))
            elif r < 0.85 and earlier:
                bad = (rng.choice((OP_INSERT, OP_READ)), rng.choice(earlier))
            elif members:
                bad = (OP_MEMBER, self.fresh(1, vals)[0])
            else:
                bad = (OP_READ, 0)
            ops.insert(at, bad[0])
            vals.insert(at, bad[1])
        return vals, ops

    def make_load_values(self):
        m, rng, c = self.m, self.rng, self.n_new[LOAD_VALUES] - 1
        length, source = ("shorter", "longer", "same")[c % 3], ("earlier", "unrelated")[(c >> 2) & 1]
        cur, top = m.size, min(m.cap, SIZE_LIMIT)
        span = dict(shorter=(2, cur - 1), longer=(cur + 1, min(top, cur + 24)), same=(max(cur, 2), min(cur, top)))[length]
        if span[0] > span[1]:
            span = (2, min(top, 12))
        vals = None
        if source == "earlier":                                # a prefix of an earlier state, not of the present one
            states = [s for s in self.history if len(s) >= span[0] and s[:span[0]] != tuple(m.vals[:span[0]])]
            if states:
                s = rng.choice(states)
                vals = list(s[1:rng.randint(span[0], min(span[1], len(s)))])
        if vals is None:
            source = "unrelated"
            vals = [self.other.pop() for _ in range(rng.randint(*span) - 1)]
        return dict(vals=tuple(vals), device=bool(c & 1), fmt=(c >> 1) % 3, source=source)

    def make_reserve(self, grow):
        m, c = self.m, self.n_new[RESERVE] - 1
        lo, hi = max(2, 1 << (m.size - 1).bit_length()), min(1 << m.depth, MAX_CAP)
        order = ("grow", "shrink", "same")
        order = order[c % 3:] + order[:c % 3]
        if grow or (self.room() < 4 and m.cap < hi):
            order = ("grow", ) + order
        for v in order:
            if v == "grow" and m.cap * 2 <= hi:
                return m.cap * 2
            if v == "shrink" and lo < m.cap:
                return lo
            if v == "same":
                return m.cap

    def make(self, kind, refusal, item=None):
        item = item or {}
        if refusal:
            return self.make_refusal(refusal, item)
        m, rng, room = self.m, self.rng, self.room()
        small = item.get("small")
        if kind in NEW_KINDS:
            c = self.n_new[kind]
            self.n_new[kind] += 1
        if kind == 3 and small:
            return Step(3, None, tuple(self.fresh(rng.randint(1, 2))), None, None)
        if kind in (BULK, APPLY_PIPE):
            vals = item.get("vals") or tuple(self.fresh(rng.randint(1, min(2 if small else 16, room))))
            arg = dict(device=bool(c & 1), item_major=bool((c >> 1) & 1)) if kind == BULK else \
                dict(host_prep=item.get("host_prep", bool(c & 1)), inputs_ready=bool((c >> 1) & 1))
            return Step(kind, None, vals, arg, None)
        if kind in (MIXED_FILT, APPLY_MIXED, MIXED_PIPE):
            members = item.get("members", bool(c & 1))
            if kind == MIXED_FILT:
                arg, noisy = dict(device=bool((c >> 1) & 1), item_major=bool((c >> 2) & 1)), True
            elif kind == APPLY_MIXED:
                arg = dict(filtered=bool((c >> 1) & 1))
                noisy = arg["filtered"]
            else:
                arg, noisy = dict(apply=bool((c >> 1) & 1)), False
            top = MIXED_MAX_OPS[self.shape.depth]
            n = rng.randint(1, 3 if small else top - 3 * noisy)
            n_ins = rng.randint(1 if small and room else 0, min(room, n, 8))
            vals, ops = self.make_block(n_ins, n, members, noisy, top)
            arg.update(ops=tuple(ops), members=members)
            return Step(kind, None, tuple(vals), arg, None)
        if kind == LOAD_VALUES:
            return Step(kind, None, None, self.make_load_values(), None)
        if kind == RESERVE:
            return Step(kind, None, None, self.make_reserve(item.get("grow")), None)
        return super().make(kind, None)

    def make_refusal(self, name, item=None):
        item = item or {}
        if name not in NEW_REFUSALS:
            return super().make_refusal(name)
        m, rng = self.m, self.rng
        self.n_refused += 1
        c, room = self.n_refused, m.cap - m.size
        if name == "plain_only":
            kind = (BULK, MIXED_FILT, APPLY_MIXED, MIXED_PIPE)[c % 4]
            vals = tuple(self.fresh(1))
            arg = dict(device=bool(c & 1), item_major=False) if kind == BULK else dict(ops=(OP_INSERT, ), members=bool(c & 2))
            arg.update({MIXED_FILT: dict(device=bool(c & 1), item_major=False), APPLY_MIXED: dict(filtered=bool(c & 1)),
                        MIXED_PIPE: dict(apply=bool(c & 1))}.get(kind, {}))
            return Step(kind, name, vals, arg, None)
        if name.startswith(("bulk", "pipe")):
            kind, what = (BULK if name.startswith("bulk") else APPLY_PIPE), name.split("_", 1)[1]
            if what == "full":
                vals = list(item.get("vals") or self.fresh(room + 1))
            else:
                good = self.fresh(min(rng.randint(2, 5), room) - 1)
                bad = dict(stored=lambda: rng.choice(m.vals[1:]), repeat=lambda: rng.choice(good), zero=lambda: 0,
                           ge_p=lambda: P + rng.randrange(3))[what]()
                vals = good + [bad]
                rng.shuffle(vals)
            arg = dict(device=bool(c & 1), item_major=bool(c & 2)) if kind == BULK else dict(host_prep=bool(c & 1), inputs_ready=False)
            return Step(kind, name, tuple(vals), arg, None)
        if name.startswith("lv"):
            if name == "lv_full":
                vals = [self.other.pop() for _ in range(m.cap)]
            else:
                vals = [self.other.pop() for _ in range(min(rng.randint(3, 8), m.cap - 1) - 1)]
                bad = dict(lv_zero=lambda: 0, lv_repeat=lambda: rng.choice(vals), lv_ge_p=lambda: P + rng.randrange(3))[name]()
                vals.insert(rng.randint(1 if name == "lv_repeat" else 0, len(vals)), bad)
                if name == "lv_ge_p" and len(vals) + 2 <= m.cap:       # a 0 as well: still NONCANONICAL, bad_pos the smaller
                    vals.insert(rng.randint(0, len(vals)), 0)
            return Step(LOAD_VALUES, name, None, dict(vals=tuple(vals), device=bool(c & 1), fmt=0 if name == "lv_ge_p" else c % 3,
                                                      source="refused"), None)
        if name.startswith("reserve"):
            cap = dict(reserve_below=lambda: max(2, 1 << ((m.size - 1).bit_length() - 1)), reserve_npot=self.npot,
                       reserve_above=lambda: 2 << m.depth)[name]()
            return Step(RESERVE, name, None, cap, None)
        kind = item.get("kind") or ((APPLY_MIXED, MIXED_PIPE) if name == "member_absent" else (MIXED_FILT, APPLY_MIXED, MIXED_PIPE))[c % (2 if name == "member_absent" else 3)]
        top = MIXED_MAX_OPS[self.shape.depth]
        n = rng.randint(2, 5)
        vals, ops = self.make_block(rng.randint(0, min(room, n, 3)), n, True, False, top)
        if name == "member_absent":
            at = rng.randint(0, len(ops))
            ops.insert(at, OP_MEMBER)
            vals.insert(at, self.fresh(1, vals)[0])
        elif OP_MEMBER not in ops:
            ops.append(OP_MEMBER)
            vals.append(vals[0])
        arg = dict(ops=tuple(ops), members=name == "member_absent")
        arg.update({MIXED_FILT: dict(device=bool(c & 1), item_major=bool(c & 2)), APPLY_MIXED: dict(filtered=name != "member_absent" and bool(c & 1)),
                    MIXED_PIPE: dict(apply=bool(c & 1))}[kind])
        return Step(kind, name, tuple(vals), arg, None)

    def script(self, number, shape, seed):
        self.shape, self.rng, self.m = shape, random.Random(seed), new_model(shape)
        self.plain = not (shape.placement or shape.partition[0])
        own = lambda s, n: [v for v in oracle_lib.synth_values(n, s) if self.m.mine(v)]
        self.pool, self.other = own(seed, 1500), own(seed ^ 0x00FF0000, 2400)
        self.specials, self.history = [], [tuple(self.m.vals)]
        self.stale_refusal = self.host_side = False
        steps, prev, queue, flight, stuck = [], None, [], [], 0
        while len(steps) < THIRD_STEPS and not (self.done() and len(steps) >= 8 and not queue):
            queue = queue or self.plan(prev, len(steps))
            if queue:
                item = queue.pop(0)
            else:
                kind, refusal = self.choose(prev, len(steps))
                if kind is None and refusal is None:
                    if len(steps) >= 8:
                        break
                    kind = self.rng.choice([k for k in NEW_KINDS if self.feasible(k)])
                item = dict(kind=kind, refusal=refusal)
            if not self.feasible(item["kind"]) if not item.get("refusal") else not self.refusal_feasible(item["refusal"]):
                queue, stuck = [], stuck + 1                   # the story has run out of room: drop the rest of it
                assert stuck < 100, f"the third pass does not reach its coverage: {item} cannot be played"
                continue
            st = self.make(item.get("kind"), item.get("refusal"), item)
            if st.refusal:
                check = item.get("check") or self.refusal_level()
                self.refusals = [r for r in self.refusals if r != st.refusal]
                if st.kind not in PIPELINED:
                    flight = []
            else:
                check = item.get("check") or self.level(st.kind)
                if prev is not None and prev.refusal:
                    self.need11.discard(st.kind)
                elif prev is not None:
                    self.need.discard((prev.kind, st.kind, prev.check))
                    self.need_any.discard((prev.kind, st.kind))
                if len(flight) >= 2 and len(set(flight)) >= 2:
                    self.need_flight.discard(st.kind)
                play(self.m, st)
                self.history.append(tuple(self.m.vals))
                flight = flight + [st.kind] if st.kind in PIPELINED else []
            if check != NO_CHECK:
                flight = []
            st = st._replace(check=check)
            steps.append(st)
            prev = st
            if not queue:
                self.host_side = False
        steps[-1] = steps[-1]._replace(check=FULL)
        return Script(f"{shape.name}_{number:02d}", shape, tuple(steps))


N_FIRST_PASS = 9                     # scripts of the first pass: the record of what ran before the mixed batch existed
N_OLD_PASSES = 14                    # scripts of the first two passes: the record of what ran before kinds 14 to 20 did
_SCRIPTS = None


def scripts():
    """the committed scripts: as many as the coverage conditions need, every shape at least once; the first pass first"""
    global _SCRIPTS
    if _SCRIPTS is None:
        g, out = _Generator(), []
        while not g.done() or len(out) < len(SHAPES):
            assert len(out) < len(SEEDS), "the generator does not reach its coverage"
            out.append(g.script(len(out), SHAPES[len(out) % len(SHAPES)], SEEDS[len(out)]))
        assert len(out) == N_FIRST_PASS
        g = _MixedGenerator()
        while not g.done():
            k = len(out) - N_FIRST_PASS
            assert k < len(MIXED_SEEDS), "the second pass does not reach its coverage"
            out.append(g.script(len(out), MIXED_SHAPES[k % len(MIXED_SHAPES)], MIXED_SEEDS[k]))
        assert len(out) == N_OLD_PASSES
        g = _ThirdGenerator()
        while not g.done() or len(out) - N_OLD_PASSES < len(THIRD_SHAPES):
            k = len(out) - N_OLD_PASSES
            assert k < len(THIRD_SEEDS), f"the third pass does not reach its coverage: {g.left()}"
            out.append(g.script(len(out), THIRD_SHAPES[THIRD_ORDER[k]], THIRD_SEEDS[k]))
        _SCRIPTS = tuple(out)
    return _SCRIPTS


def third_pass_d32():
    """the script of the third pass the thread and quad contexts play as well: the first at depth 32 with all seven new kinds"""
    return next(s for s in scripts()[N_OLD_PASSES:] if s.shape.depth == 32 and
                {st.kind for st in s.steps if not st.refusal} >= set(NEW_KINDS))


def flights(script):
    """Per step the pipelined kinds still in flight when it enters, counted by the model: a batch of kind 3, 15 or 18
    stays in flight until the next LIGHT / FULL check or the wait of a synchronous call; a refused pipelined call leaves
    them alone, any other refused call is taken to have waited."""
    out, flight = [], []
    for st in script.steps:
        out.append(tuple(flight))
        if st.refusal:
            flight = flight if st.kind in PIPELINED else []
        else:
            flight = flight + [st.kind] if st.kind in PIPELINED else []
        if st.check != NO_CHECK:
            flight = []
    return out


def caps(script):
    """the capacity before every step (reserve changes it)"""
    m, out = new_model(script.shape), []
    for st in script.steps:
        out.append(m.cap)
        try:
            play(m, st)
        except Refused:
            pass
    return out


# ---------------------------------------------------------------- the oracle's tree of a model state
_ROOTS, _PROOFS, _ROWS, _READ_ROWS = {}, {}, {}, {}


def pre_arr(pre):
    """[(val, next_val, next_idx)] -> uint8 [n, 3, 32]"""
    return ints_to_arr([x for p in pre for x in p]).reshape(-1, 3, 32)


def _handle(orc, shape, vals):
    h = orc.sparse_new(shape.depth, shape.cap)
    orc.sparse_set_index_base(h, index_base(shape))
    if len(vals) > 1:
        rc = orc.sparse_load(h, pre_arr(new_model(shape, vals).preimages(range(len(vals)))))
        assert rc == 0, f"the oracle refuses the model's list of {len(vals)} leaves: {rc}"
    return h


def _note(orc, h, shape, vals, proofs):
    key = (shape, tuple(vals))
    _ROOTS[key] = orc.sparse_root(h)
    if proofs and key not in _PROOFS:
        _PROOFS[key] = np.stack([orc.sparse_proof(h, shape.depth, i) for i in range(shape.cap)])


def oracle_root(shape, vals):
    key = (shape, tuple(vals))
    if key not in _ROOTS:
        orc = oracle_lib.load()
        h = _handle(orc, shape, vals)
        _note(orc, h, shape, vals, False)
        orc.sparse_free(h)
    return _ROOTS[key]


def oracle_proofs(shape, vals):
    """uint8 [cap, depth, 32]: the proof of every local leaf index of the state"""
    key = (shape, tuple(vals))
    if key not in _PROOFS:
        orc = oracle_lib.load()
        h = _handle(orc, shape, vals)
        _note(orc, h, shape, vals, True)
        orc.sparse_free(h)
    return _PROOFS[key]


def oracle_rows(shape, before, acc):
    """the imt_insert_out rows of inserting `acc` one by one into the oracle's tree of state `before` (siblings
    item-major [n, depth, 32], low_index global): the fields test_gpu_rewind.compare_rows compares"""
    key = (shape, tuple(before), tuple(acc))
    if key in _ROWS:
        return _ROWS[key]
    orc, depth, base, n = oracle_lib.load(), shape.depth, index_base(shape), len(acc)
    h = _handle(orc, shape, before)
    rec = dict(low_index=np.empty(n, np.uint64), is_largest=np.empty(n, np.uint8), low_leaf=np.empty((n, 3, 32), np.uint8),
               new_leaf=np.empty((n, 3, 32), np.uint8), old_root=np.empty((n, 32), np.uint8),
               interim_root=np.empty((n, 32), np.uint8), new_root=np.empty((n, 32), np.uint8),
               low_sib=np.empty((n, depth, 32), np.uint8), new_sib=np.empty((n, depth, 32), np.uint8))
    try:
        for k, v in enumerate(acc):
            old = orc.sparse_root(h)
            r = orc.sparse_insert(h, depth, v)
            assert r["rc"] == 0, (shape.name, k, r["rc"])
            rec["low_index"][k], rec["is_largest"][k], rec["low_leaf"][k] = r["low"] + base, r["largest"], r["low_leaf"]
            nl = r["low_leaf"].copy()
            nl[0] = ints_to_arr([v])[0]
            rec["new_leaf"][k] = nl
            rec["old_root"][k] = ints_to_arr([old])[0]
            rec["interim_root"][k] = ints_to_arr([r["interim_root"]])[0]
            rec["new_root"][k] = ints_to_arr([r["new_root"]])[0]
            rec["low_sib"][k], rec["new_sib"][k] = r["low_proof"], r["new_proof"]
        _note(orc, h, shape, tuple(before) + tuple(acc), False)
    finally:
        orc.sparse_free(h)
    _ROWS[key] = rec
    return rec


def oracle_read_rows(shape, before, step, carried=None):
    """the imt_read_out rows of the READs of mixed-batch `step` on the oracle's tree of state `before`: one walk on one
    handle, sparse_insert at every INSERT, and at every READ sparse_root and sparse_proof of the low leaf the model names
    (siblings item-major [n_reads, depth, 32], low_index global); the oracle's preimage of that leaf must be the model's"""
    vals, ops = step.vals, step.arg["ops"]
    if carried is not None:                                    # a filtered twin: the operations it carried out
        vals, ops = tuple(vals[p] for p in carried), tuple(ops[p] for p in carried)
    key = (shape, tuple(before), vals, ops)
    if key in _READ_ROWS:
        return _READ_ROWS[key]
    orc, depth, base = oracle_lib.load(), shape.depth, index_base(shape)
    m = new_model(shape, before)
    n = len(ops) - ops.count(OP_INSERT)
    rec = dict(low_index=np.empty(n, np.uint64), is_largest=np.empty(n, np.uint8), low_leaf=np.empty((n, 3, 32), np.uint8),
               root=np.empty((n, 32), np.uint8), low_sib=np.empty((n, depth, 32), np.uint8))
    h, q = _handle(orc, shape, before), 0
    try:
        for p, (v, op) in enumerate(zip(vals, ops)):
            if op == OP_INSERT:
                m.insert([v])
                assert orc.sparse_insert(h, depth, v)["rc"] == 0, (shape.name, p)
                continue
            low, leaf, largest = m.nm_witness(v) if op == OP_READ else m.member_witness(v)      # a MEMBER: the leaf that holds v
            pre = orc.sparse_preimage(h, low - base)
            assert (pre == pre_arr([leaf])[0]).all(), f"{shape.name}: the oracle's leaf {low} at operation {p} is not the model's"
            rec["low_index"][q], rec["is_largest"][q], rec["low_leaf"][q] = low, largest, pre
            rec["root"][q] = ints_to_arr([orc.sparse_root(h)])[0]
            rec["low_sib"][q] = orc.sparse_proof(h, depth, low - base)
            q += 1
    finally:
        orc.sparse_free(h)
    _READ_ROWS[key] = rec
    return rec
