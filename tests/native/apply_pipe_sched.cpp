// The pipeline rule of imt_apply_pipe.hpp against a model of what every launch reads and writes.
//
// A launch is the set of stored levels it reads and the set it writes (bit l = level l, bit `depth` = the root row).
// Batches run on different streams, so the only order there is between launches is: stream order inside a batch, and
// "launch x starts after the launch that records event e of the batch before, and after everything before THAT launch
// on its stream".  A hazard is a pair of launches of different batches that conflict (read-after-write,
// write-after-read, write-after-write) and are not ordered, earlier batch first, by the closure of those edges.
//
// Prints one line per question:
//   rule_hazards <n>       hazards under imt::apipe::waits over every depth <= 6, every chain of two and three
//                          batches, every kind and every l0 of each (0 is the only right answer)
//   rule_cases <n>         how many chains that was
//   spaced1_hazards <n>    the same check of apply behind apply when AP_LEVEL l waits for the launch that WROTE level l
//                          in the batch in front -- the one-level spacing of the witness pipeline (must be > 0)
//   unordered_hazards <n>  the same with no waits at all (must be > 0)
//   first_hazard ...       the first hazard of the rule, if any
#include <cstdint>
#include <cstdio>
#include <vector>

#include "imt_apply_pipe.hpp"

using namespace imt::apipe;

namespace {

struct Node {
    Launch x;
    uint32_t reads, writes;
};
struct Batch {
    Kind kind;
    unsigned l0;
    std::vector<Node> launches;     // in stream order
};

// the model: written from what the kernels touch (imt_itree.cpp: apply_hashes, witness_sweep), not from the header
Batch make_batch(Kind kind, unsigned l0, unsigned depth) {
    Batch b{kind, l0, {}};
    auto bit = [](unsigned l) { return (uint32_t)1 << l; };
    if (kind == APPLY) {
        b.launches.push_back({{AP_LEVEL, 0}, 0, bit(0)});
        for (unsigned l = 1; l < l0; l++) b.launches.push_back({{AP_LEVEL, l}, bit(l - 1), bit(l)});
        b.launches.push_back({{AP_CHAIN, 0}, bit(l0 - 1), 0});
        uint32_t w = 0;
        for (unsigned l = l0; l <= depth; l++) w |= bit(l);
        b.launches.push_back({{AP_STORE, 0}, 0, w});
        return b;
    }
    for (unsigned l = 0; l < l0; l++) b.launches.push_back({{WI_LEVEL, l}, bit(l), bit(l)});
    for (unsigned l = l0; l < depth; l++) {
        if (l + 1 == depth) b.launches.push_back({{WI_OLD_ROOT, 0}, bit(depth), 0});
        b.launches.push_back({{WI_UPPER, l}, 0, bit(l + 1) | (l == l0 ? bit(l) : 0)});
    }
    if (l0 == depth) b.launches.push_back({{WI_OLD_ROOT, 0}, bit(depth), 0});
    b.launches.push_back({{WI_ROOTS, 0}, 0, l0 == depth ? bit(depth) : 0});
    return b;
}

typedef Event (*Rule)(Kind, unsigned, Kind, unsigned, unsigned, Launch);

Event rule_header(Kind p, unsigned pl0, Kind c, unsigned l0, unsigned depth, Launch x) { return waits(p, pl0, c, l0, depth, x); }
Event rule_none(Kind, unsigned, Kind, unsigned, unsigned, Launch) { return {EV_NONE, 0}; }

// index of the launch of b that records event e; launches.size() - 1 for DONE; -1: nobody records it
int recorder(const Batch& b, unsigned depth, Event e) {
    if (e.type == EV_DONE) return (int)b.launches.size() - 1;
    for (size_t i = 0; i < b.launches.size(); i++) {
        const Event r = records(b.kind, b.l0, depth, b.launches[i].x);
        if (r.type == EV_LEVEL && r.l == e.l) return (int)i;
    }
    return -1;
}

// the witness pipeline's spacing, for apply behind apply: AP_LEVEL l starts when the batch in front has WRITTEN level l
// (its own AP_LEVEL l, or its store from its l0 up); everything else as the header has it
int spaced1_recorder(const Batch& prev, unsigned depth, Launch x) {
    if (x.type != AP_LEVEL) return recorder(prev, depth, waits(APPLY, prev.l0, APPLY, 0, depth, x));
    if (x.l >= prev.l0) return (int)prev.launches.size() - 1;
    return (int)x.l;        // AP_LEVEL l is launch number l of an apply batch
}

struct Result {
    uint64_t hazards = 0;
    bool have_first = false;
    char first[256];
};

// chain[0] runs first.  mode 0: `rule`; mode 1: spaced1_recorder (apply chains only)
void check_chain(const std::vector<Batch>& chain, unsigned depth, Rule rule, int mode, Result& res) {
    std::vector<int> base(chain.size());
    int N = 0;
    for (size_t b = 0; b < chain.size(); b++) {
        base[b] = N;
        N += (int)chain[b].launches.size();
    }
    // before[i] bit j: launch j finishes before launch i starts (N <= 3 * 16 < 64)
    std::vector<uint64_t> before(N, 0);
    for (size_t b = 0; b < chain.size(); b++)
        for (size_t i = 0; i < chain[b].launches.size(); i++) {
            uint64_t m = 0;
            if (i > 0) m |= before[base[b] + i - 1] | ((uint64_t)1 << (base[b] + i - 1));
            if (b > 0) {
                const Batch& p = chain[b - 1];
                int r;
                if (mode == 1) {
                    r = spaced1_recorder(p, depth, chain[b].launches[i].x);
                } else {
                    const Event e = rule(p.kind, p.l0, chain[b].kind, chain[b].l0, depth, chain[b].launches[i].x);
                    r = e.type == EV_NONE ? -2 : recorder(p, depth, e);
                    if (r == -1) {      // a wait for an event nobody records is a stale event: no order at all, and a finding
                        res.hazards++;
                        if (!res.have_first) {
                            res.have_first = true;
                            std::snprintf(res.first, sizeof res.first, "depth %u: batch %zu launch %zu waits for LEVEL %u, which batch %zu never records",
                                          depth, b, i, e.l, b - 1);
                        }
                    }
                }
                if (r >= 0) m |= before[base[b - 1] + r] | ((uint64_t)1 << (base[b - 1] + r));
            }
            before[base[b] + i] = m;
        }
    for (size_t a = 0; a < chain.size(); a++)
        for (size_t b = a + 1; b < chain.size(); b++)
            for (size_t i = 0; i < chain[a].launches.size(); i++)
                for (size_t j = 0; j < chain[b].launches.size(); j++) {
                    const Node &u = chain[a].launches[i], &v = chain[b].launches[j];
                    const bool conflict = (u.writes & v.reads) || (u.reads & v.writes) || (u.writes & v.writes);
                    if (!conflict) continue;
                    if (before[base[b] + j] >> (base[a] + i) & 1) continue;
                    res.hazards++;
                    if (!res.have_first) {
                        res.have_first = true;
                        std::snprintf(res.first, sizeof res.first,
                                      "depth %u: batch %zu (kind %d, l0 %u) launch %zu (type %d, l %u) and batch %zu (kind %d, l0 %u) launch %zu "
                                      "(type %d, l %u)",
                                      depth, a, (int)chain[a].kind, chain[a].l0, i, (int)u.x.type, u.x.l, b, (int)chain[b].kind, chain[b].l0, j,
                                      (int)v.x.type, v.x.l);
                    }
                }
}

}  // namespace

int main() {
    Result rule, spaced, none;
    uint64_t cases = 0;
    for (unsigned depth = 1; depth <= 6; depth++) {
        std::vector<Batch> all;
        for (int k = 0; k < 2; k++)
            for (unsigned l0 = 1; l0 <= depth; l0++) all.push_back(make_batch((Kind)k, l0, depth));
        for (const Batch& a : all)
            for (const Batch& b : all) {
                check_chain({a, b}, depth, rule_header, 0, rule);
                cases++;
                if (a.kind == APPLY && b.kind == APPLY) {
                    check_chain({a, b}, depth, nullptr, 1, spaced);
                    check_chain({a, b}, depth, rule_none, 0, none);
                }
                for (const Batch& c : all) {
                    check_chain({a, b, c}, depth, rule_header, 0, rule);
                    cases++;
                }
            }
    }
    std::printf("rule_hazards %llu\n", (unsigned long long)rule.hazards);
    std::printf("rule_cases %llu\n", (unsigned long long)cases);
    std::printf("spaced1_hazards %llu\n", (unsigned long long)spaced.hazards);
    std::printf("unordered_hazards %llu\n", (unsigned long long)none.hazards);
    if (rule.have_first) std::printf("first_hazard %s\n", rule.first);
    if (spaced.have_first) std::printf("first_spaced1_hazard %s\n", spaced.first);
    return 0;
}
