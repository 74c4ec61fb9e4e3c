"""TreeModel with presence reads (TEST INFRASTRUCTURE ONLY): IMT_OP_MEMBER under IMT_MEMBER_OPS, from include/imt.h
"PRESENCE READS".

MemberModel adds the third kind to the walk of a mixed block and the filtered twin's rule, written from the header and
not from the library's restatements (member_neighbours, mixed_carried): a MEMBER of v asks lookup(v) of the list at
that moment, the answer must be PRESENT at a leaf L, and its row is L, L's preimage then and whether L points at
nothing.  tree_model.py is not edited; a block without MEMBERs goes through the same code and gives what TreeModel
gives (tests/test_member_logic.py asserts that on its exhaustive set).
"""
from oracle_lib import P
from tree_model import (NEW, NONE, OP_INSERT, OP_READ, PRESENT, REPEATED, ZERO, Refused, TreeModel)

OP_MEMBER = 2
KIND = "IRM"


class MemberModel(TreeModel):
    def member_witness(self, v):
        """(leaf, its preimage, is_largest) of the leaf that holds v now; refused if none does or v is 0"""
        if v >= P:
            raise Refused("NONCANONICAL")
        status, leaf = self.lookup(v)
        if status != PRESENT:
            raise Refused("VALUE")
        pre = self.preimages([leaf - self.index_base])[0]
        assert pre[0] == v
        return leaf, pre, int(pre[1] == 0)

    def mixed(self, vals, ops, members=True):
        """TreeModel.mixed with MEMBERs: returns (the values inserted, [(position, leaf index, leaf preimage, is_largest,
        INSERTs before it)] of the operations that are no INSERT, in block order -- the rows of `rd`).  members=False is
        the call without the flag: op byte 2 is an argument error."""
        vals, ops = list(vals), list(ops)
        if self.index_base or self.part_mod > 1 or any(op > (OP_MEMBER if members else OP_READ) for op in ops):
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
                elif op == OP_READ:
                    reads.append((p, ) + self.nm_witness(v) + (len(acc), ))
                else:
                    reads.append((p, ) + self.member_witness(v) + (len(acc), ))
        except Refused:
            self.rewind(start)
            raise Refused("VALUE", p)
        return acc, reads

    def mixed_classify(self, vals, ops):
        """(status, carried positions) of the filtered twins, nothing changed.  status[p] says what the VALUE is at that
        place whichever kind the operation is: ZERO, PRESENT (stored before the call), REPEATED (p > f(v), f(v) the
        smallest position whose operation is an INSERT of v), else NEW.  An INSERT or a READ is carried out iff NEW, a
        MEMBER iff PRESENT or REPEATED."""
        vals, ops = list(vals), list(ops)
        if any(v >= P for v in vals):
            raise Refused("NONCANONICAL")
        f = {}
        for p, (v, op) in enumerate(zip(vals, ops)):
            if op == OP_INSERT:
                f.setdefault(v, p)
        status, carried = [], []
        for p, (v, op) in enumerate(zip(vals, ops)):
            s = ZERO if v == 0 else PRESENT if v in self.where else REPEATED if v in f and p > f[v] else NEW
            status.append(s)
            if (s in (PRESENT, REPEATED)) if op == OP_MEMBER else s == NEW:
                carried.append(p)
        return status, carried, f

    def mixed_filtered(self, vals, ops):
        """The filtered twin: (status, leaf_index, carried positions, what mixed() returns for the carried operations).
        leaf_index[p]: a carried INSERT's new leaf, a carried READ's low leaf as of its place, a MEMBER's leaf (PRESENT:
        the stored one, REPEATED: the one the INSERT at f(v) wrote), the sentinel for ZERO, NONE for a skipped MEMBER;
        a skipped INSERT or READ as TreeModel.classify has it."""
        vals, ops = list(vals), list(ops)
        status, carried, f = self.mixed_classify(vals, ops)
        if self.size + sum(ops[p] == OP_INSERT for p in carried) > self.cap:
            raise Refused("FULL")
        stored = dict(self.where)
        start = self.size
        acc, reads = self.mixed([vals[p] for p in carried], [ops[p] for p in carried])      # never refused: that is the rule
        new_leaf = {v: self.index_base + start + r for r, v in enumerate(acc)}
        low_of = {carried[k]: low for k, low, _, _, _ in reads}
        leaf = []
        for p, (v, op, s) in enumerate(zip(vals, ops, status)):
            if s == ZERO:
                leaf.append(self.index_base)
            elif s == PRESENT:
                leaf.append(self.index_base + stored[v])
            elif s == REPEATED:
                leaf.append(new_leaf[vals[f[v]]])
            elif op == OP_INSERT:
                leaf.append(new_leaf[v])
            elif op == OP_READ:
                leaf.append(low_of[p])
            else:
                leaf.append(NONE)
        return status, leaf, carried, (acc, reads)
