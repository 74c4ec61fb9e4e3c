// member_neighbours.cpp -- TEST INFRASTRUCTURE: the rules of a mixed block that holds presence reads (IMT_OP_MEMBER under
// IMT_MEMBER_OPS) on the CPU: member_neighbours beside read_neighbours (csrc/imt_prep_logic.hpp) and the filtered twin's
// mixed_carried / mixed_filter_op_leaf (csrc/imt_filter_logic.hpp), over arrays built the way prep::mixed_ranks,
// mixed_check and mixed_filter build them on the device.  A stand-alone program: it reads blocks from standard input and
// prints what the rules say of every operation; tests/test_member_logic.py feeds it and compares with the model's walk.
//
// Input, repeated until end of file (values are up to 64 hex digits, most significant first):
//     S M n
//     <M stored values in leaf order, leaf 0 = the sentinel 0>
//     <n lines: op value>            op: 0 = INSERT, 1 = READ, 2 = MEMBER
// Output per block:
//     n lines "kind low succ err"    the strict call: low / succ are rows of the value array (succ -1 = none), err the OP_*
//                                    bits of that operation
//     "bad <smallest offending position or -1>"
//     n lines "status leaf carried"  the filtered call: leaf -1 = UINT64_MAX
//     "counts <carried INSERTs> <carried READs and MEMBERs> <bad of the strict rules on the carried operations>"
//     one line "kind low succ" per carried operation that is no INSERT, from the strict rules on the carried operations
//     "end"
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "imt_filter_logic.hpp"

using namespace imt::prep;

static bool parse256(const char* hex, uint8_t* out) {
    const size_t len = std::strlen(hex);
    if (len == 0 || len > 64) return false;
    std::memset(out, 0, 32);
    for (size_t i = 0; i < len; i++) {
        const char ch = hex[len - 1 - i];
        unsigned d;
        if (ch >= '0' && ch <= '9') d = ch - '0';
        else if (ch >= 'a' && ch <= 'f') d = 10 + ch - 'a';
        else return false;
        out[i / 2] |= (uint8_t)(d << (4 * (i & 1)));        // little-endian bytes
    }
    return true;
}

static int levels_for(uint32_t n) {
    int k = 1;
    while ((1u << k) <= n) k++;
    return k;
}

struct Strict {
    std::vector<uint32_t> low, succ, at;       // at[p]: where operation p's neighbours are
    std::vector<int> err;
    uint32_t n_ins = 0, bad = OP_NONE;
};

// prep::mixed_ranks + mixed_check over n operations; val has room for M + n rows and rows [M, M + n_ins) are written
static Strict strict_rules(uint8_t* val, const uint32_t* sorted_old, uint32_t M, const uint8_t* vals, const uint8_t* op,
                           uint32_t n) {
    Strict s;
    std::vector<uint32_t> flag(n), rank(n), ipos(n), iota(n);
    for (uint32_t p = 0; p < n; p++) {
        flag[p] = op[p] == OP_INSERT;
        rank[p] = s.n_ins;
        s.n_ins += flag[p];
    }
    const uint32_t n_ins = s.n_ins;
    s.err.assign(n, 0);
    for (uint32_t p = 0; p < n; p++) {
        s.err[p] |= op_value_class(vals + (size_t)p * 32, 0, 0);
        if (!flag[p]) continue;
        std::memcpy(val + (size_t)(M + rank[p]) * 32, vals + (size_t)p * 32, 32);
        iota[rank[p]] = M + rank[p];
        ipos[rank[p]] = p;
    }
    std::vector<uint32_t> bsorted(iota.begin(), iota.begin() + n_ins);
    std::sort(bsorted.begin(), bsorted.end(), [&](uint32_t a, uint32_t b) {
        const uint8_t *x = val + (size_t)a * 32, *y = val + (size_t)b * 32;
        return lt256(x, y) || (a < b && !lt256(y, x));
    });
    const int levels = levels_for(n_ins);
    // exactly the sizes the kernels may touch: the sanitizer build reports a read beyond them
    std::vector<uint32_t> gap(n_ins), st((size_t)levels * n_ins);
    s.low.assign(n, 0);
    s.succ.assign(n, 0);
    s.at.assign(n, 0);
    for (uint32_t j = 0; j < n_ins; j++) {
        gap[j] = count_below(val, sorted_old, M, val + (size_t)bsorted[j] * 32);
        st[j] = bsorted[j] - M;
        if (insert_is_duplicate(val, sorted_old, M, bsorted.data(), j, gap[j])) s.err[ipos[st[j]]] |= OP_DUPLICATE;
    }
    for (int k = 1; k < levels; k++)
        for (uint32_t j = 0; j + (1u << k) <= n_ins; j++)
            st[(size_t)k * n_ins + j] = std::min(st[(size_t)(k - 1) * n_ins + j], st[(size_t)(k - 1) * n_ins + j + (1u << (k - 1))]);
    for (uint32_t j = 0; j < n_ins; j++) {     // k_neighbours
        const uint32_t g = gap[j], t = st[j];
        const uint32_t jl = nearest_smaller_left(st.data(), n_ins, levels, j);
        const uint32_t jr = nearest_smaller_right(st.data(), n_ins, levels, j);
        s.low[t] = (jl < n_ins && gap[jl] == g) ? bsorted[jl] : sorted_old[g > 0 ? g - 1 : 0];
        s.succ[t] = (jr < n_ins && gap[jr] == g) ? bsorted[jr] : (g < M ? sorted_old[g] : OP_NONE);
    }
    for (uint32_t p = 0; p < n; p++) {         // k_mixed_reads
        s.at[p] = flag[p] ? rank[p] : n_ins + (p - rank[p]);
        if (flag[p]) continue;
        const uint8_t* x = vals + (size_t)p * 32;
        const ReadAnswer a =
            op[p] == OP_MEMBER
                ? member_neighbours(x, rank[p], val, sorted_old, M, bsorted.data(), gap.data(), st.data(), n_ins, levels, 0, 0)
                : read_neighbours(x, rank[p], val, sorted_old, M, bsorted.data(), gap.data(), st.data(), n_ins, levels, 0, 0);
        s.err[p] |= a.err;
        s.low[s.at[p]] = a.low;
        s.succ[s.at[p]] = a.succ;
    }
    for (uint32_t p = 0; p < n; p++)
        if (s.err[p] && p < s.bad) s.bad = p;
    return s;
}

static long or_none(uint32_t x) { return x == OP_NONE ? -1L : (long)x; }

int main() {
    unsigned M, n;
    char tag[8], hex[128];
    int blocks = 0;
    const char kind[] = "IRM";
    while (std::scanf("%7s %u %u", tag, &M, &n) == 3) {
        if (tag[0] != 'S' || M == 0) return 2;
        // 8-byte aligned rows: the rules read values as 64-bit limbs
        std::vector<uint64_t> val_store((size_t)(M + n) * 4), in_store((size_t)n * 4 + 4), acc_store((size_t)n * 4 + 4);
        uint8_t* val = reinterpret_cast<uint8_t*>(val_store.data());
        uint8_t* vals = reinterpret_cast<uint8_t*>(in_store.data());
        uint8_t* acc = reinterpret_cast<uint8_t*>(acc_store.data());
        std::vector<uint8_t> op(n);
        for (unsigned i = 0; i < M; i++)
            if (std::scanf("%127s", hex) != 1 || !parse256(hex, val + (size_t)i * 32)) return 2;
        for (unsigned p = 0; p < n; p++) {
            unsigned o;
            if (std::scanf("%u %127s", &o, hex) != 2 || o > OP_MEMBER || !parse256(hex, vals + (size_t)p * 32)) return 2;
            op[p] = (uint8_t)o;
        }
        std::vector<uint32_t> sorted_old(M);
        for (unsigned i = 0; i < M; i++) sorted_old[i] = i;
        std::sort(sorted_old.begin(), sorted_old.end(),
                  [&](uint32_t a, uint32_t b) { return lt256(val + (size_t)a * 32, val + (size_t)b * 32); });

        // ---- the strict call ----
        const Strict s = strict_rules(val, sorted_old.data(), M, vals, op.data(), n);
        for (unsigned p = 0; p < n; p++)
            std::printf("%c %u %ld %d\n", kind[op[p]], s.low[s.at[p]], or_none(s.succ[s.at[p]]), s.err[p]);
        std::printf("bad %ld\n", or_none(s.bad));

        // ---- the filtered call: class, sort, rank, the two scans, compact; then the strict rules on what is carried out ----
        std::vector<uint8_t> st(n), aop;
        std::vector<uint32_t> ord(n), aux(n, 0), flag_ins(n), flag_rd(n), rank_ins(n), rank_rd(n), apos;
        for (unsigned p = 0; p < n; p++) ord[p] = p;
        std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return mixed_pos_less(vals, op.data(), a, b); });
        for (unsigned j = 0; j < n; j++) {
            const uint32_t p = ord[j];
            st[p] = mixed_filter_rank(vals, op.data(), ord.data(), j, filter_class(vals + (size_t)p * 32, 0, 0), val,
                                      sorted_old.data(), M, &aux[p]);
            flag_ins[p] = op[p] == OP_INSERT && mixed_carried(op[p], st[p]);
            flag_rd[p] = op[p] != OP_INSERT && mixed_carried(op[p], st[p]);
        }
        uint32_t ni = 0, nr = 0;
        for (unsigned p = 0; p < n; p++) {
            rank_ins[p] = ni;
            rank_rd[p] = nr;
            ni += flag_ins[p];
            nr += flag_rd[p];
        }
        std::vector<uint64_t> leaf(n, 0);
        for (unsigned p = 0; p < n; p++) {       // k_mixed_filter_compact
            const bool carried = mixed_carried(op[p], st[p]);
            if (carried) {
                std::memcpy(acc + (size_t)aop.size() * 32, vals + (size_t)p * 32, 32);
                aop.push_back(op[p]);
                apos.push_back(p);
            }
            if (!(carried && op[p] == OP_READ)) leaf[p] = mixed_filter_op_leaf(op[p], st[p], aux[p], rank_ins.data(), p, 0, M);
        }
        const uint32_t n_acc = (uint32_t)aop.size();
        const Strict f = strict_rules(val, sorted_old.data(), M, acc, aop.data(), n_acc);
        for (uint32_t k = 0; k < n_acc; k++)     // k_mixed_filter_reads
            if (aop[k] == OP_READ) leaf[apos[k]] = f.low[f.at[k]];
        for (unsigned p = 0; p < n; p++)
            std::printf("%u %ld %d\n", (unsigned)st[p], leaf[p] == LEAF_NONE ? -1L : (long)leaf[p], (int)mixed_carried(op[p], st[p]));
        std::printf("counts %u %u %ld\n", ni, nr, or_none(f.bad));
        for (uint32_t k = 0; k < n_acc; k++)
            if (aop[k] != OP_INSERT) std::printf("%c %u %ld\n", kind[aop[k]], f.low[f.at[k]], or_none(f.succ[f.at[k]]));
        std::printf("end\n");
        blocks++;
    }
    std::printf("blocks %d ok\n", blocks);
    return 0;
}
