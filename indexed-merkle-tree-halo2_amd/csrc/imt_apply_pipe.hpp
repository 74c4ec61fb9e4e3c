// imt_apply_pipe.hpp -- how consecutive batches on the tree's pipeline streams are ordered against each other.
//
// A pipelined batch runs on its own stream; what keeps it off the toes of the batch before is a stream wait, per launch,
// for one event of that batch's plan set.  This header says which one, for either kind of batch behind either kind, and
// which event each launch records.  imt_itree.cpp takes its waits from here and from nowhere else;
// tests/native/apply_pipe_sched.cpp checks them against every conflict of every pair and triple of batches.
//
// The launches of a batch with occupied height l0 (2^l0 >= size after the batch, 1 <= l0 <= depth), in stream order:
//
//   apply (imt_apply.hpp), pipelined form              reads stored level        writes stored level
//     AP_LEVEL 0          the touched leaves           -                         0
//     AP_LEVEL l, l < l0  the touched nodes of level l l - 1                     l
//     AP_CHAIN            node 0 of levels l0..depth   l0 - 1 (nodes 0 and 1)    - (rows of the plan set)
//     AP_STORE            those rows into the tree     -                         l0 .. depth
//   witness (imt_sweep.hpp)
//     WI_LEVEL l, l < l0  sweep + write-back           l (siblings)              l
//     WI_OLD_ROOT         the root the batch found     depth                     -
//     WI_UPPER l, l >= l0 node 0 against empty         -                         l + 1, and l when l == l0
//     WI_ROOTS            every event's root           -                         depth when l0 == depth
//
// An apply batch hashes straight into the stored tree, with no time-versioned copies, so the batch behind it must not
// overwrite a level the batch in front still has to READ: AP_LEVEL l + 1 of the batch in front reads level l, which
// AP_LEVEL l of the batch behind writes -- with ascending values the new node is the very sibling.  So an apply batch
// runs TWO launches behind the one in front, where the witness sweep, which reads and writes level l in one launch, runs
// one behind.
//
// The events of a plan set: LEVEL l = "stored level l is final and this batch no longer reads it", DONE = the batch's last
// operation (behind its copy of the root into the plan set).  A batch records LEVEL l
//   apply:    after AP_LEVEL l + 1 for l < l0 - 1, after AP_CHAIN for l = l0 - 1; levels from l0 up are final at DONE;
//   witness:  after WI_LEVEL l's write-back for l < l0, after WI_UPPER l for l >= l0 (as it always has).
#pragma once

namespace imt {
namespace apipe {

enum Kind : int { APPLY = 0, WITNESS = 1 };
enum LaunchType : int { AP_LEVEL = 0, AP_CHAIN, AP_STORE, WI_LEVEL, WI_OLD_ROOT, WI_UPPER, WI_ROOTS };
struct Launch {
    LaunchType type;
    unsigned l;         // AP_LEVEL, WI_LEVEL, WI_UPPER: the level; otherwise unused
};
enum EventType : int { EV_NONE = 0, EV_LEVEL, EV_DONE };
struct Event {
    EventType type;
    unsigned l;         // EV_LEVEL: which
};

// The event of the previous batch's plan set that launch x of this batch waits for before it starts (EV_NONE: stream order
// behind this batch's earlier launches already covers it).
inline Event waits(Kind prev, unsigned prev_l0, Kind cur, unsigned l0, unsigned depth, Launch x) {
    (void)l0;
    (void)depth;
    const Event none{EV_NONE, 0}, done{EV_DONE, 0};
    if (cur == APPLY) {
        switch (x.type) {
        case AP_LEVEL:
            // Writes level l and reads l - 1.  LEVEL l of the batch in front: its reader of level l has finished, and in
            // its stream order so have its writers of l and of l - 1.  From its l0 up its store writes the level: DONE.
            // (Behind a witness batch LEVEL l is its write-back of level l, behind that of l - 1.)
            return x.l < prev_l0 ? Event{EV_LEVEL, x.l} : done;
        case AP_CHAIN:
            // reads level l0 - 1, which AP_LEVEL l0 - 1 before it on this stream wrote behind the wait above
            return none;
        case AP_STORE:
            // levels l0 .. depth and the root: behind everything the batch in front does up there
            return done;
        default:
            return done;
        }
    }
    switch (x.type) {
    case WI_LEVEL:
        return x.l < prev_l0 ? Event{EV_LEVEL, x.l} : done;
    case WI_OLD_ROOT:
        return done;
    case WI_UPPER:
        // behind a witness batch: it stored node l + 1 (and node l, at its own l0) from its launch of this level;
        // an apply batch stores all of them at its end
        return prev == WITNESS && x.l >= prev_l0 ? Event{EV_LEVEL, x.l} : done;
    case WI_ROOTS:
        return none;        // WI_OLD_ROOT before it on this stream has waited for DONE
    default:
        return done;
    }
}

// The event launch x records when it has finished (EV_NONE: none; DONE is recorded by the caller behind the last launch).
inline Event records(Kind cur, unsigned l0, unsigned depth, Launch x) {
    (void)depth;
    const Event none{EV_NONE, 0};
    if (cur == APPLY) {
        if (x.type == AP_LEVEL && x.l >= 1 && x.l < l0) return Event{EV_LEVEL, x.l - 1};
        if (x.type == AP_CHAIN) return Event{EV_LEVEL, l0 - 1};
        return none;
    }
    if (x.type == WI_LEVEL || x.type == WI_UPPER) return Event{EV_LEVEL, x.l};
    return none;
}

}  // namespace apipe
}  // namespace imt
