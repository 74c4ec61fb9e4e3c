// emul_gadget.cpp -- TEST-ONLY host build of the per-item code of the gadget kernels (csrc/imt_gadget_device.hpp: the
// 256-bit helpers, the row emitters, the less_than item and the insert / non-inclusion item), so that `-m "not gpu"`
// tests can compare it with the oracle and the Python model at every lookup width without a GPU
// (tests/test_gadget_widths_cpu.py).  The entry points loop over the items as the kernels' grids do.
// With -DEMUL_GADGET_MAIN it is also a program of its own that repeats the comparisons against liboracle.so at every
// width, for a run under -fsanitize=address,undefined.  Not part of the shipped library.
#include "imt_gadget_device.hpp"

using namespace imt::gadget;

// rows of is_less_than for n pairs a[n][32], b[n][32] (canonical); row r of item i at trace + r * row_stride +
// i * item_stride; lt_out [n] may be null.  Returns 0, or -3 for a width outside 1..28.
extern "C" int emul_gadget_less_than(const uint8_t* a, const uint8_t* b, size_t n, unsigned lookup_bits, uint8_t* trace,
                                     uint64_t row_stride, uint64_t item_stride, uint8_t* lt_out) {
    if (lookup_bits < 1 || lookup_bits > 28) return -3;
    for (size_t i = 0; i < n; i++) {
        const uint32_t lt = less_than_item(a, b, i, lookup_bits, trace, row_stride, item_stride);
        if (lt_out) lt_out[i] = (uint8_t)lt;
    }
    return 0;
}

// the glue rows of n insert_leaf calls (whole_insert: new_leaf [n][3][32], pairs [4][depth][n][2][32]) or of n
// verify_non_inclusion calls (new_leaf = the bare values [n][32], pairs [1][depth][n][2][32], new_path_index unused);
// everything canonical, pairs as the C entries build them: (left, right) of every path hash
extern "C" int emul_gadget_insert(const uint8_t* low_leaf, const uint64_t* low_index, const uint8_t* new_leaf,
                                  const uint64_t* new_path_index, const uint8_t* is_largest, const uint8_t* pairs, unsigned depth,
                                  unsigned lookup_bits, size_t n, int whole_insert, uint8_t* trace, uint64_t row_stride,
                                  uint64_t item_stride) {
    if (lookup_bits < 1 || lookup_bits > 28 || depth < 1 || depth > 64) return -3;
    for (size_t i = 0; i < n; i++)
        insert_gadget_item(low_leaf, low_index, new_leaf, whole_insert ? 96u : 32u, whole_insert ? new_path_index : low_index,
                           is_largest, pairs, depth, lookup_bits, n, i, whole_insert, trace, row_stride, item_stride);
    return 0;
}

// the four rows of gate.is_equal(a[i], b[i]) -- a - b mod p, z, 1 / (a - b) (1 if equal), z -- into rows[n][4][32]
extern "C" void emul_gadget_is_equal(const uint8_t* a, const uint8_t* b, size_t n, uint8_t* rows) {
    for (size_t i = 0; i < n; i++) {
        Out o{rows, 32, 128, i, 0};
        emit_is_equal(o, load256(a + i * 32), load256(b + i * 32));
    }
}

#ifdef EMUL_GADGET_MAIN
// ---- the stand-alone form: every width, against liboracle.so ----
#include <cstdio>
#include <vector>
extern "C" {
#include "../../oracle/imt_oracle.h"
}

namespace {

struct Row { uint8_t b[32]; };
int g_failures;
void expect(bool cond, const char* what, unsigned lb, long which) {
    if (cond) return;
    std::fprintf(stderr, "FAIL %s: lookup_bits %u, case %ld\n", what, lb, which);
    g_failures++;
}
// p - 1, little-endian
const uint8_t P_MINUS_1[32] = {0x00, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                               0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};
uint64_t g_x = 0x9E3779B97F4A7C15ull;
Row rnd253() {                                               // xorshift64 bytes, below 2^253 < p
    Row r;
    for (int k = 0; k < 32; k++) {
        g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17;
        r.b[k] = (uint8_t)(g_x >> 32);
    }
    r.b[31] &= 0x1f;
    return r;
}
Row pow2(unsigned e) {
    Row r{};
    r.b[e / 8] = (uint8_t)(1u << (e % 8));
    return r;
}
Row pow2m1(unsigned e) {                                     // 2^e - 1
    Row r{};
    for (unsigned k = 0; k < e / 8; k++) r.b[k] = 0xff;
    if (e % 8) r.b[e / 8] = (uint8_t)((1u << (e % 8)) - 1u);
    return r;
}
Row small(uint64_t v) {
    Row r{};
    std::memcpy(r.b, &v, 8);
    return r;
}

// the operand pairs of one width: fixed edges, the limb boundaries of both halves, random pairs, shared high halves
void pairs_of(unsigned lb, std::vector<Row>& a, std::vector<Row>& b) {
    a.clear(); b.clear();
    auto add = [&](const Row& x, const Row& y) { a.push_back(x); b.push_back(y); };
    Row pm1;
    std::memcpy(pm1.b, P_MINUS_1, 32);
    add(small(0), small(0)); add(small(0), small(1)); add(small(1), small(0)); add(small(5), small(5));
    add(pm1, pm1); add(pm1, small(0)); add(small(0), pm1);
    add(pow2m1(128), pow2(128)); add(pow2(128), pow2m1(128)); add(pow2m1(128), small(0)); add(small(0), pow2m1(128));
    add(pow2m1(253), small(0)); add(small(0), pow2m1(253));
    for (unsigned e = 0; e < 128; e += lb) {
        add(pow2(e), pow2m1(e)); add(pow2m1(e), pow2(e));
        if (128 + e <= 253) { add(pow2(128 + e), pow2m1(128 + e)); add(pow2m1(128 + e), pow2(128 + e)); }
    }
    for (int j = 0; j < 12; j++) add(rnd253(), rnd253());
    for (int j = 0; j < 6; j++) {                            // same high half: the low halves decide
        Row x = rnd253(), y = rnd253();
        std::memcpy(y.b + 16, x.b + 16, 16);
        add(x, y);
    }
    const Row e = rnd253();
    add(e, e);
}

void check_less_than(unsigned lb) {
    std::vector<Row> a, b;
    pairs_of(lb, a, b);
    const size_t n = a.size(), rows = orc_less_than_trace_rows(lb);
    expect(rows == 4 * ((128 + lb - 1) / lb + 1) + 27, "row count", lb, -1);
    // exactly rows * n: one row more, or an item past the end, is an overflow the sanitizer reports
    std::vector<Row> rm(rows * n), im(rows * n), owit(rows), ocells(8 * rows);
    std::vector<orc_trace_cell> odesc(ocells.size());
    std::vector<uint8_t> lt(n), lt2(n);
    expect(emul_gadget_less_than(a[0].b, b[0].b, n, lb, rm[0].b, n * 32, 32, lt.data()) == 0, "row-major status", lb, -1);
    expect(emul_gadget_less_than(a[0].b, b[0].b, n, lb, im[0].b, 32, rows * 32, lt2.data()) == 0, "item-major status", lb, -1);
    for (size_t i = 0; i < n; i++) {
        size_t nc = 0, nw = 0;
        uint32_t orow = 0;
        expect(orc_less_than_trace(a[i].b, b[i].b, lb, ocells[0].b, odesc.data(), ocells.size(), &nc, owit[0].b, owit.size(), &nw,
                                   &orow) == 0 && nw == rows, "oracle trace", lb, (long)i);
        bool same = true, same_im = true;
        for (size_t r = 0; r < rows; r++) {
            same &= std::memcmp(rm[r * n + i].b, owit[r].b, 32) == 0;
            same_im &= std::memcmp(im[i * rows + r].b, owit[r].b, 32) == 0;
        }
        expect(same, "less_than rows, row-major", lb, (long)i);
        expect(same_im, "less_than rows, item-major", lb, (long)i);
        expect(lt[i] == owit[orow].b[0] && lt2[i] == lt[i] && lt[i] == (uint8_t)orc_is_less_than_limbs(a[i].b, b[i].b),
               "less_than result", lb, (long)i);
    }
}

// (left, right) of every hash of the path of `leaf` at `index` over `proof`: out[depth][n][2], item i
void chain_pairs(Row* out, size_t n, size_t i, Row cur, uint64_t index, const Row* proof, unsigned depth) {
    for (unsigned l = 0; l < depth; l++) {
        Row* pp = out + ((size_t)l * n + i) * 2;
        const bool left_child = ((index >> l) & 1) == 0;
        pp[0] = left_child ? cur : proof[l];
        pp[1] = left_child ? proof[l] : cur;
        orc_hash2(cur.b, pp[0].b, pp[1].b);
    }
}
Row hash3(const Row* leaf) {
    Row h;
    orc_hash_var(h.b, leaf[0].b, 3);
    return h;
}

// real insertions into a sparse tree of the oracle, every third one turned into a witness the circuit rejects
void check_insert(unsigned lb, unsigned depth, size_t n) {
    orc_sparse* t = nullptr;
    expect(orc_sparse_new(&t, depth, 8) == 0, "sparse tree", lb, depth);
    std::vector<Row> low(3 * n), nw(3 * n), lproof(depth * n), nproof(depth * n), nval(n);
    std::vector<uint64_t> li(n), ni(n), npi(n);
    std::vector<uint8_t> lg(n);
    for (size_t i = 0; i < n; i++) {
        Row v = rnd253();
        int largest = 0;
        expect(orc_sparse_insert(t, v.b, &li[i], (uint8_t(*)[32])low[3 * i].b, &largest, nullptr, nullptr, lproof[depth * i].b,
                                 nproof[depth * i].b) == 0, "sparse insert", lb, (long)i);
        nw[3 * i] = v; nw[3 * i + 1] = low[3 * i + 1]; nw[3 * i + 2] = low[3 * i + 2];
        ni[i] = npi[i] = 1 + i;
        lg[i] = (uint8_t)largest;
        if (i % 3 == 1) lg[i] ^= 1;                                       // is_largest flipped
        if (i % 3 == 2 && (i & 1)) std::swap(nw[3 * i], low[3 * i]);      // new value and low.val swapped
        if (i % 3 == 2 && !(i & 1)) npi[i] = ni[i] ^ 1;                   // new_path_index != new_index
        nval[i] = nw[3 * i];
    }
    orc_sparse_free(t);
    const size_t ps = (size_t)depth * n * 2;
    std::vector<Row> pairs(4 * ps);
    const Row zero3[3] = {};
    for (size_t i = 0; i < n; i++) {
        const Row relinked[3] = {low[3 * i], nw[3 * i], small(ni[i])};
        chain_pairs(&pairs[0], n, i, hash3(&low[3 * i]), li[i], &lproof[depth * i], depth);
        chain_pairs(&pairs[ps], n, i, hash3(relinked), li[i], &lproof[depth * i], depth);
        chain_pairs(&pairs[2 * ps], n, i, hash3(zero3), npi[i], &nproof[depth * i], depth);
        chain_pairs(&pairs[3 * ps], n, i, hash3(&nw[3 * i]), npi[i], &nproof[depth * i], depth);
    }
    const size_t rows = orc_insert_gadget_rows(depth, lb), head = orc_non_inclusion_gadget_rows(depth, lb);
    std::vector<Row> got(rows * n), got_head(head * n), want(rows);
    std::vector<orc_column_segment> segs(8 * depth + 16);
    expect(emul_gadget_insert(low[0].b, li.data(), nw[0].b, npi.data(), lg.data(), pairs[0].b, depth, lb, n, 1, got[0].b, n * 32,
                              32) == 0, "insert status", lb, depth);
    expect(emul_gadget_insert(low[0].b, li.data(), nval[0].b, nullptr, lg.data(), pairs[0].b, depth, lb, n, 0, got_head[0].b, 32,
                              head * 32) == 0, "non-inclusion status", lb, depth);
    for (size_t i = 0; i < n; i++) {
        size_t nrows = 0, nsegs = 0;
        expect(orc_insert_gadget_trace((const uint8_t(*)[32])low[3 * i].b, li[i], lproof[depth * i].b, (const uint8_t(*)[32])nw[3 * i].b,
                                       ni[i], npi[i], nproof[depth * i].b, lg[i], depth, lb, want[0].b, rows, &nrows, segs.data(),
                                       segs.size(), &nsegs) == 0 && nrows == rows, "oracle insert rows", lb, (long)i);
        bool same = true, same_head = true;
        for (size_t r = 0; r < rows; r++) same &= std::memcmp(got[r * n + i].b, want[r].b, 32) == 0;
        expect(same, "insert rows", lb, (long)i);
        expect(orc_non_inclusion_gadget_trace((const uint8_t(*)[32])low[3 * i].b, li[i], lproof[depth * i].b, nval[i].b, lg[i], depth, lb,
                                              want[0].b, rows, &nrows, segs.data(), segs.size(), &nsegs) == 0 && nrows == head,
               "oracle non-inclusion rows", lb, (long)i);
        for (size_t r = 0; r < head; r++) same_head &= std::memcmp(got_head[i * head + r].b, want[r].b, 32) == 0;
        expect(same_head, "non-inclusion rows", lb, (long)i);
    }
}

}  // namespace

int main() {
    orc_poseidon_init();
    Row x = small(1), y = small(2), out[4];
    expect(emul_gadget_less_than(x.b, y.b, 1, 0, out[0].b, 32, 32, nullptr) == -3 &&
           emul_gadget_less_than(x.b, y.b, 1, 29, out[0].b, 32, 32, nullptr) == -3, "widths outside 1..28", 0, 0);
    for (unsigned lb = 1; lb <= 28; lb++) {
        check_less_than(lb);
        check_insert(lb, 3, 6);
        if (lb == 1 || lb == 18 || lb == 28) check_insert(lb, 32, 3);
    }
    if (g_failures) { std::fprintf(stderr, "%d checks failed\n", g_failures); return 1; }
    std::printf("gadget host checks ok: lookup widths 1..28, less_than, insert and non-inclusion rows\n");
    return 0;
}
#endif
