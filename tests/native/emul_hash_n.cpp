// emul_hash_n.cpp -- TEST-ONLY host build of the sponge stages for 1..16 inputs (imt_device.hpp::hash_sponge,
// imt_trace_device.hpp::hash_sponge_trace) and of the cell map for any length (imt_trace_layout.cpp), so that
// `-m "not gpu"` tests can compare them with the oracle on a machine without a GPU (tests/test_hash_n_cpu.py).
// With -DEMUL_HASH_N_MAIN it is also a program of its own that runs the same comparisons against liboracle.so, for a
// run under -fsanitize=address,undefined.  Not part of the shipped library.
#include "imt_device.hpp"
#include "imt_trace_device.hpp"
#include "imt_params.hpp"
#include "imt_ctx.hpp"
#include <cstring>
#include <string>

using namespace imt;
static HostPoseidon* g_hp;
static dev::PoseidonConsts g_consts;
static dev::TraceConsts g_tconsts;
static imt_ctx* g_fake;          // a context that only carries the tables: the layout calls read nothing else

extern "C" int emul_hn_init(void) {
    if (g_hp) return 0;
    g_hp = new HostPoseidon();
    std::string err;
    if (!g_hp->init(err)) return -1;
    g_hp->fill_consts(g_consts);
    g_hp->fill_trace_consts(g_tconsts);
    g_fake = new imt_ctx();
    if (!g_fake->hp.init(err)) return -12;
    return 0;
}

namespace {
// input j of the one hash at `in` ([len][32], 16-byte aligned)
struct InputAt {
    const uint8_t* in;
    unsigned fmt_in;
    bool* ok;
    void operator()(unsigned j, dev::Fe& x) const { *ok &= dev::load_fe(g_consts, x, in + (size_t)j * 32, fmt_in); }
};
}  // namespace

// out = the hash of in[len][32] through the value stage; 0, or -5 for an input >= p
extern "C" int emul_hn_hash(const uint8_t* in, unsigned len, uint8_t* out, unsigned fmt_in, unsigned fmt_out) {
    bool ok = true;
    dev::Fe o;
    dev::hash_sponge(g_consts, o, len, InputAt{in, fmt_in, &ok});
    dev::store_fe(g_consts, out, o, fmt_out);
    return ok ? 0 : -5;
}
// rows [n_rows][32] in fmt_out through the trace stage; returns the number of rows written, or -5
extern "C" int emul_hn_trace(const uint8_t* in, unsigned len, uint8_t* rows, unsigned fmt_in, unsigned fmt_out) {
    bool ok = true;
    dev::TraceSink o{rows, 32};
    InputAt load{in, fmt_in, &ok};
    if (fmt_out == dev::FMT_MONT256) dev::hash_sponge_trace<dev::FMT_MONT256>(g_consts, g_tconsts, o, len, load);
    else if (fmt_out == dev::FMT_DEVICE) dev::hash_sponge_trace<dev::FMT_DEVICE>(g_consts, g_tconsts, o, len, load);
    else dev::hash_sponge_trace<dev::FMT_CANONICAL>(g_consts, g_tconsts, o, len, load);
    return ok ? (int)((o.p - rows) / 32) : -5;
}
extern "C" void emul_hn_convert(const uint8_t* in, uint8_t* out, unsigned fmt_in, unsigned fmt_out) {
    dev::Fe x;
    dev::load_fe(g_consts, x, in, fmt_in);
    dev::store_fe(g_consts, out, x, fmt_out);
}
// the product's cell maps without a GPU: the general call, and the fixed-length call it must agree with at 2 and 3
extern "C" int emul_hn_layout(unsigned len, imt_trace_cell* cells, size_t cells_cap, size_t* n_cells, void* constants,
                              size_t const_cap, size_t* n_constants, uint32_t* out_row, unsigned flags) {
    return imt_hash_n_trace_layout(g_fake, len, cells, cells_cap, n_cells, constants, const_cap, n_constants, out_row, flags);
}
extern "C" int emul_hn_layout23(int arity, imt_trace_cell* cells, size_t cells_cap, size_t* n_cells, void* constants,
                                size_t const_cap, size_t* n_constants, uint32_t* out_row, unsigned flags) {
    return imt_hash_trace_layout(g_fake, arity, cells, cells_cap, n_cells, constants, const_cap, n_constants, out_row, flags);
}

#ifdef EMUL_HASH_N_MAIN
// ---- the stand-alone form: every length, five input vectors, against liboracle.so ----
#include <cstdio>
#include <vector>
extern "C" {
#include "../../oracle/imt_oracle.h"
}

namespace {

struct alignas(16) Row { uint8_t b[32]; };
int g_failures;
void expect(bool cond, const char* what, unsigned len, int which) {
    if (cond) return;
    std::fprintf(stderr, "FAIL %s: len %u, vector %d\n", what, len, which);
    g_failures++;
}
// p - 1, little-endian
const uint8_t P_MINUS_1[32] = {0x00, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                               0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};

void fill_inputs(std::vector<Row>& in, unsigned len, int which) {
    in.assign(len, Row{});
    uint64_t x = 0x9E3779B97F4A7C15ull * (uint64_t)(which + 1) + len;
    for (unsigned j = 0; j < len; j++) {
        if (which == 0) continue;                                        // [0] * len
        if (which == 1) { std::memcpy(in[j].b, P_MINUS_1, 32); continue; }   // [p - 1] * len
        for (int k = 0; k < 32; k++) {                                   // synthetic: xorshift64 bytes, below 2^253 < p
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            in[j].b[k] = (uint8_t)(x >> 32);
        }
        in[j].b[31] &= 0x1f;
    }
}

void check_len(unsigned len) {
    const size_t rows = imt_hash_n_trace_rows(len);
    for (int which = 0; which < 5; which++) {
        std::vector<Row> in, in_f(len);
        fill_inputs(in, len, which);
        const uint8_t* inp = in[0].b;
        Row want_hash;
        expect(orc_hash_var(want_hash.b, inp, len) == 0, "oracle hash", len, which);
        // the oracle's column
        size_t nc = 0, nw = 0;
        uint32_t orow = 0;
        std::vector<Row> ocells(12 * 2256), owit(rows + 8);
        std::vector<orc_trace_cell> odesc(ocells.size());
        expect(orc_hash_trace(inp, (int)len, ocells[0].b, odesc.data(), ocells.size(), &nc, owit[0].b, owit.size(), &nw, &orow) == 0,
               "oracle trace", len, which);
        expect(nw == rows && orow == rows - 4, "row count", len, which);
        expect(nc == (size_t)2256 * (len / 2) + 2250 + 3 * (len & 1u), "cell count", len, which);
        expect(std::memcmp(owit[orow].b, want_hash.b, 32) == 0, "oracle output row", len, which);
        // value and trace stages in every format (inputs converted to it, results converted back)
        for (unsigned fmt = 0; fmt < 3; fmt++) {
            for (unsigned j = 0; j < len; j++) emul_hn_convert(in[j].b, in_f[j].b, 0, fmt);
            Row h, hc;
            expect(emul_hn_hash(in_f[0].b, len, h.b, fmt, fmt) == 0, "value stage status", len, which);
            emul_hn_convert(h.b, hc.b, fmt, 0);
            expect(std::memcmp(hc.b, want_hash.b, 32) == 0, "value stage", len, which);
            std::vector<Row> got(rows);                                  // exactly rows: one row more is an overflow
            expect(emul_hn_trace(in_f[0].b, len, got[0].b, fmt, fmt) == (int)rows, "trace stage rows", len, which);
            bool same = true;
            for (size_t r = 0; r < rows && r < nw; r++) {
                Row c;
                emul_hn_convert(got[r].b, c.b, fmt, 0);
                same &= std::memcmp(c.b, owit[r].b, 32) == 0;
            }
            expect(same, "trace stage", len, which);
        }
        // the cell map against the oracle's, and the column rebuilt from it
        size_t pc = 0, pk = 0;
        uint32_t prow = 0;
        expect(emul_hn_layout(len, nullptr, 0, &pc, nullptr, 0, &pk, &prow, 0) == 0, "layout sizes", len, which);
        std::vector<imt_trace_cell> cells(pc);
        std::vector<Row> consts(pk);
        expect(emul_hn_layout(len, cells.data(), pc, &pc, consts[0].b, pk, &pk, &prow, 0) == 0, "layout", len, which);
        expect(pc == nc && prow == orow, "layout counts", len, which);
        bool map_ok = pc == nc, col_ok = pc == nc;
        for (size_t i = 0; i < pc && i < nc; i++) {
            const imt_trace_cell& c = cells[i];
            map_ok &= c.kind == odesc[i].kind && c.gate == odesc[i].gate && c.region == odesc[i].region;
            if (c.kind != IMT_CELL_CONST) map_ok &= c.index == odesc[i].index;
            Row v{};
            if (c.kind == IMT_CELL_CONST) v = consts[c.index];
            else if (c.kind == IMT_CELL_INPUT) { if (c.index < len) v = in[c.index]; else map_ok = false; }
            else if (c.kind == IMT_CELL_INIT) { if (c.index == 0) v.b[8] = 1; }
            else { if (c.index < nw) v = owit[c.index]; else map_ok = false; }
            col_ok &= std::memcmp(v.b, ocells[i].b, 32) == 0;
        }
        expect(map_ok, "layout cells", len, which);
        expect(col_ok, "rebuilt column", len, which);
    }
}

}  // namespace

int main() {
    if (emul_hn_init() != 0) { std::fprintf(stderr, "table generation failed\n"); return 2; }
    orc_poseidon_init();
    expect(imt_hash_n_trace_rows(0) == 0 && imt_hash_n_trace_rows(IMT_HASH_MAX_INPUTS + 1) == 0, "rows outside 1..16", 0, 0);
    expect(emul_hn_layout(0, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0) == IMT_ERR_ARG, "layout of 0 inputs", 0, 0);
    expect(emul_hn_layout(17, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0) == IMT_ERR_ARG, "layout of 17 inputs", 17, 0);
    for (unsigned len = 1; len <= IMT_HASH_MAX_INPUTS; len++) check_len(len);
    if (g_failures) { std::fprintf(stderr, "%d checks failed\n", g_failures); return 1; }
    std::printf("hash_n host checks ok: lengths 1..%d, 5 vectors, 3 formats\n", IMT_HASH_MAX_INPUTS);
    return 0;
}
#endif
