// emul_device.cpp -- TEST-ONLY host build of the device arithmetic (imt_device.hpp) and
// of the host table generator, so that `-m "not gpu"` tests can compare the radix-2^29
// Montgomery code, the optimised Poseidon schedule and the index kernels' per-element
// logic with the oracle on a machine without a GPU.  Not part of the shipped library.
#include "imt_device.hpp"
#include "imt_trace_device.hpp"
#include "imt_params.hpp"
#include <cstring>
#include <string>

using namespace imt;
static HostPoseidon* g_hp;
static dev::PoseidonConsts g_consts;
static dev::TraceConsts g_tconsts;

extern "C" int emul_init(void) {
    if (g_hp) return 0;
    g_hp = new HostPoseidon();
    std::string err;
    if (!g_hp->init(err)) return -1;
    g_hp->fill_consts(g_consts);
    g_hp->fill_trace_consts(g_tconsts);
    return 0;
}
extern "C" int emul_consts_size(void) { return (int)sizeof(dev::PoseidonConsts); }

// out = hash2/hash3 of canonical little-endian inputs, through the device code path
extern "C" int emul_hash(const uint8_t* in, int arity, uint8_t* out, unsigned fmt_in, unsigned fmt_out) {
    dev::Fe a, b, c, o;
    bool ok = dev::load_fe(g_consts, a, in, fmt_in);
    ok &= dev::load_fe(g_consts, b, in + 32, fmt_in);
    c = a;
    if (arity == 3) ok &= dev::load_fe(g_consts, c, in + 64, fmt_in);
    dev::hash23(g_consts, o, a, b, c, arity == 3);
    {   // the variant k_sweep uses (third input parked in a stash until the second permutation) must agree
        dev::Fe o2;
        uint32_t stash[dev::NL * 4];
        for (int i = 0; i < dev::NL; i++) stash[i * 4] = c.v[i];
        dev::hash23_stashed(g_consts, o2, a, b, arity == 3, stash, 4);
        if (!dev::fe_eq(o, o2)) return -12;
    }
    dev::store_fe(g_consts, out, o, fmt_out);
    return ok ? 0 : -5;
}
extern "C" int emul_permute(const uint8_t* in, uint8_t* out) {
    dev::Fe s[3];
    bool ok = true;
    for (int i = 0; i < 3; i++) ok &= dev::load_fe(g_consts, s[i], in + 32 * i, dev::FMT_CANONICAL);
    dev::permute(g_consts, s, g_consts.rc_full[0]);
    for (int i = 0; i < 3; i++) { dev::canonicalize(s[i]); dev::store_fe(g_consts, out + 32 * i, s[i], dev::FMT_CANONICAL); }
    return ok ? 0 : -5;
}
// r = a*b (field product of canonical inputs) via mont_mul / mont_sqr
extern "C" void emul_mul(const uint8_t* a, const uint8_t* b, uint8_t* out, int use_sqr) {
    dev::Fe x, y, r;
    dev::load_fe(g_consts, x, a, dev::FMT_CANONICAL);
    dev::load_fe(g_consts, y, b, dev::FMT_CANONICAL);
    if (use_sqr) dev::mont_sqr(r, x); else dev::mont_mul(r, x, y);
    dev::canonicalize(r);
    dev::store_fe(g_consts, out, r, dev::FMT_CANONICAL);
}
extern "C" void emul_convert(const uint8_t* in, uint8_t* out, unsigned fmt_in, unsigned fmt_out) {
    dev::Fe x;
    dev::load_fe(g_consts, x, in, fmt_in);
    dev::store_fe(g_consts, out, x, fmt_out);
}
// host-side (product) Poseidon used for table self-checks
extern "C" void emul_host_hash(const uint8_t* in, int arity, uint8_t* out) {
    HFr a, b, c;
    g_hp->F.from_bytes(a, in);
    g_hp->F.from_bytes(b, in + 32);
    HFr h;
    if (arity == 3) { g_hp->F.from_bytes(c, in + 64); h = g_hp->hash3(a, b, c); }
    else h = g_hp->hash2(a, b);
    g_hp->F.to_bytes(out, h);
}

// ---- index logic of the batch-insertion sweep (imt_sweep.hpp), one level on the host ----
#include "imt_sweep.hpp"
extern "C" void emul_merge_level(const uint32_t* node, const uint32_t* time, const uint32_t* rs, const uint32_t* re,
                                 uint32_t total, uint32_t* o_node, uint32_t* o_time, uint32_t* o_rs, uint32_t* o_re,
                                 uint32_t* o_from, int32_t* o_sibsrc, uint32_t* o_node_below) {
    sweep::LevelTable in{node, time, rs, re};
    sweep::LevelOut out{o_node, o_time, o_rs, o_re, o_from, o_sibsrc, o_node_below, nullptr};
    for (uint32_t k = 0; k < total; k++) sweep::merge_element(in, out, k, total);
}

// ---- GPU-prepare logic (imt_prep_logic.hpp) on the host ----
#include "imt_prep_logic.hpp"
extern "C" void emul_sparse_table(uint32_t* st, uint32_t n, int levels) {
    for (int k = 1; k < levels; k++)
        for (uint32_t j = 0; j + (1u << k) <= n; j++) {
            uint32_t a = st[(uint64_t)(k - 1) * n + j], b = st[(uint64_t)(k - 1) * n + j + (1u << (k - 1))];
            st[(uint64_t)k * n + j] = a < b ? a : b;
        }
}
extern "C" uint32_t emul_nsl(const uint32_t* st, uint32_t n, int levels, uint32_t j) {
    return imt::prep::nearest_smaller_left(st, n, levels, j);
}
extern "C" uint32_t emul_nsr(const uint32_t* st, uint32_t n, int levels, uint32_t j) {
    return imt::prep::nearest_smaller_right(st, n, levels, j);
}
// snapshot check of imt_itree_load: OR of load_check_rank over every rank
extern "C" int emul_load_check(const uint8_t* pre, uint32_t n, uint64_t base, const uint32_t* idx) {
    int e = 0;
    for (uint32_t r = 0; r < n; r++) e |= prep::load_check_rank(pre, n, base, idx, r);
    return e;
}
extern "C" uint32_t emul_count_below(const uint8_t* val, const uint32_t* sorted, uint32_t M, const uint8_t* x) {
    return imt::prep::count_below(val, sorted, M, x);
}

// ---- f1: the witness-trace device code (imt_trace_device.hpp) on the host: rows [n_rows][32] in fmt_out ----
extern "C" int emul_hash_trace(const uint8_t* in, int arity, uint8_t* rows, unsigned fmt_in, unsigned fmt_out) {
    dev::Fe a, b, c;
    bool ok = dev::load_fe(g_consts, a, in, fmt_in);
    ok &= dev::load_fe(g_consts, b, in + 32, fmt_in);
    c = a;
    if (arity == 3) ok &= dev::load_fe(g_consts, c, in + 64, fmt_in);
    dev::TraceSink o{rows, 32};
    if (fmt_out == dev::FMT_MONT256) dev::hash_trace<dev::FMT_MONT256>(g_consts, g_tconsts, o, a, b, c, arity == 3);
    else if (fmt_out == dev::FMT_DEVICE) dev::hash_trace<dev::FMT_DEVICE>(g_consts, g_tconsts, o, a, b, c, arity == 3);
    else dev::hash_trace<dev::FMT_CANONICAL>(g_consts, g_tconsts, o, a, b, c, arity == 3);
    return ok ? (int)((o.p - rows) / 32) : -5;
}
// store_mont256 alone: 9 normalised limbs of a value below 4p -> the 32 bytes it stores (value / 32 mod p)
extern "C" void emul_store_mont256(const uint32_t* limbs, uint8_t* out) {
    dev::Fe a;
    for (int i = 0; i < dev::NL; i++) a.v[i] = limbs[i];
    alignas(16) uint8_t row[32];
    dev::store_mont256(row, a);
    std::memcpy(out, row, 32);
}
// the product's cell layout (imt_trace_layout.cpp) without a GPU: a context that only carries the tables
#include "imt_ctx.hpp"
extern "C" int emul_trace_layout(int arity, imt_trace_cell* cells, size_t cells_cap, size_t* n_cells, void* constants,
                                 size_t const_cap, size_t* n_constants, uint32_t* out_row, unsigned flags) {
    static imt_ctx* fake = nullptr;
    if (!fake) {
        fake = new imt_ctx();
        std::string err;
        if (!fake->hp.init(err)) return -12;
    }
    return imt_hash_trace_layout(fake, arity, cells, cells_cap, n_cells, constants, const_cap, n_constants, out_row, flags);
}
// f3: the cell layout of one is_less_than (imt_gadget_layout.cpp), the same way
extern "C" int emul_less_than_layout(int lookup_bits, imt_trace_cell* cells, size_t cells_cap, size_t* n_cells, void* constants,
                                     size_t const_cap, size_t* n_constants, uint32_t* out_row, unsigned flags) {
    static imt_ctx* fake = nullptr;
    if (!fake) {
        fake = new imt_ctx();
        std::string err;
        if (!fake->hp.init(err)) return -12;
    }
    return imt_less_than_trace_layout(fake, (unsigned)lookup_bits, cells, cells_cap, n_cells, constants, const_cap, n_constants,
                                      out_row, flags);
}

// ---- raw limbs in and out, no canonical check (tests/test_fe_forms.py) ----
// the constant tables as the device sees them
extern "C" void emul_consts_raw(uint32_t* out) { std::memcpy(out, &g_consts, sizeof g_consts); }
extern "C" int emul_trace_consts_size(void) { return (int)sizeof(dev::TraceConsts); }
extern "C" void emul_trace_consts_raw(uint32_t* out) { std::memcpy(out, &g_tconsts, sizeof g_tconsts); }
// The C++ form each assembly form replaces (numbering: tests/fe_model.py FORMS).  in: [n][slots][9], the operand slots
// in call order (a0, b0, a1, b1, .., addend; one slot for a squaring or a REDC); out: [n][9].
extern "C" int emul_form(int form, const uint32_t* in, uint32_t* out, size_t n) {
    for (size_t j = 0; j < n; j++) {
        dev::Fe x[9] = {}, r;
        const int slots[13] = {2, 1, 6, 8, 5, 1, 3, 2, 3, 1, 2, 3, 6};
        if (form < 0 || form >= 13) return -1;
        for (int s = 0; s < slots[form]; s++)
            for (int i = 0; i < dev::NL; i++) x[s].v[i] = in[(j * slots[form] + s) * dev::NL + i];
        dev::Fe a[4], b[4];
        for (int t = 0; t < 4; t++) { a[t] = x[2 * t]; b[t] = x[2 * t + 1]; }
        switch (form) {
            case 0: dev::mont_dot<1, false, true>(r, a, b, a[0]); break;           // mul_vv
            case 1: dev::mont_sqr(r, x[0]); break;                                  // sqr_v
            case 2: dev::mont_dot<3, false, true>(r, a, b, a[0]); break;           // dot3_uc
            case 3: dev::mont_dot<4, false, true>(r, a, b, a[0]); break;           // dot4_uc
            case 4: dev::mont_dot<2, true, false>(r, a, b, x[4]); break;           // dot2_add_uc_narrow
            case 5: dev::mont_dot<1, false, false>(r, &x[0], &x[0], x[0]); break;  // sqr_v_narrow
            case 6: dev::mont_dot<1, true, false>(r, a, b, x[2]); break;           // mul_vv_adds_narrow
            case 7: dev::mont_dot<1, false, false>(r, a, b, a[0]); break;          // mul_uc_narrow
            case 8: dev::mont_dot<1, true, false>(r, a, b, x[2]); break;           // mul_uc_add_narrow
            case 9: dev::mont_redc(r, x[0]); break;                                 // redc_v_narrow
            case 10: dev::mont_dot<1, false, false>(r, a, b, a[0]); break;         // mul_vv_narrow
            case 11: dev::mont_dot<1, true, false>(r, a, b, x[2]); break;          // mul_vv_add_narrow
            case 12: dev::mont_dot<3, false, false>(r, a, b, a[0]); break;         // dot3_vv_narrow
        }
        for (int i = 0; i < dev::NL; i++) out[j * dev::NL + i] = r.v[i];
    }
    return 0;
}
// one permutation of permute() from raw entry lanes [n][3][9] (first_rc = rc_full[0]); the raw exit lanes, before any
// canonicalize
extern "C" void emul_permute_raw(const uint32_t* in, uint32_t* out, size_t n) {
    for (size_t j = 0; j < n; j++) {
        dev::Fe s[3];
        for (int l = 0; l < 3; l++)
            for (int i = 0; i < dev::NL; i++) s[l].v[i] = in[(j * 3 + l) * dev::NL + i];
        dev::permute(g_consts, s, g_consts.rc_full[0]);
        for (int l = 0; l < 3; l++)
            for (int i = 0; i < dev::NL; i++) out[(j * 3 + l) * dev::NL + i] = s[l].v[i];
    }
}
// The helpers the forms feed, on raw limbs / words (names as in tests/native/fe_forms.hip): in [n][in_words],
// out [n][out_words]
extern "C" int emul_helper(const char* name, const uint32_t* in, unsigned in_words, uint32_t* out, unsigned out_words,
                           size_t n) {
    const std::string h(name);
    for (size_t j = 0; j < n; j++) {
        const uint32_t* I = in + j * in_words;
        uint32_t* O = out + j * out_words;
        dev::Fe a, b, r;
        for (int i = 0; i < dev::NL; i++) a.v[i] = in_words >= (unsigned)dev::NL ? I[i] : 0;
        alignas(16) uint32_t w[8];
        std::memcpy(w, I, 32);
        if (h == "canonicalize") dev::canonicalize(a);
        else if (h == "fold_p") dev::fold_p(a);
        else if (h == "normalize") dev::normalize(a);
        else if (h == "cond_sub_p_shl0") dev::cond_sub_p_shl<0>(a);
        else if (h == "cond_sub_p_shl1") dev::cond_sub_p_shl<1>(a);
        else if (h == "cond_sub_p_shl2") dev::cond_sub_p_shl<2>(a);
        else if (h == "cond_sub_p_shl3") dev::cond_sub_p_shl<3>(a);
        else if (h == "cond_sub_p_shl4") dev::cond_sub_p_shl<4>(a);
        else if (h == "csub0") dev::csub<0>(a);
        else if (h == "csub1") dev::csub<1>(a);
        else if (h == "t_add") {
            for (int i = 0; i < dev::NL; i++) b.v[i] = I[dev::NL + i];
            dev::t_add(r, a, b);
            a = r;
        } else if (h == "pack") { dev::pack(w, a); std::memcpy(O, w, 32); continue; }
        else if (h == "unpack") dev::unpack(a, w);
        else if (h.rfind("load_fe", 0) == 0) {
            O[dev::NL] = dev::load_fe(g_consts, a, w, (unsigned)(h[7] - '0')) ? 1u : 0u;
        } else if (h.rfind("store_fe", 0) == 0) { dev::store_fe(g_consts, w, a, (unsigned)(h[8] - '0')); std::memcpy(O, w, 32); continue; }
        else if (h == "store_mont256") { dev::store_mont256(w, a); std::memcpy(O, w, 32); continue; }
        else return -1;
        for (int i = 0; i < dev::NL; i++) O[i] = a.v[i];
    }
    return 0;
}
