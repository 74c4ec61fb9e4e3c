// imt_device.hpp -- gfx950 device code: bn256::Fr in radix 2^29 and the Poseidon
// T=3 / R_F=8 / R_P=57 permutation + rate-2 sponge used by every kernel.
//
// Replaces, on the device, the arithmetic behind the reference call sites
//   hash.update(..); hash.squeeze_and_reset()   /root/reference/src/utils.rs:46-47,96-100
//   hasher.hash_fix_len_array(ctx, gate, &inp)  /root/reference/src/indexed_merkle_tree.rs:92,194,271-275,299-303
// (pse-poseidon / halo2-base, un-vendored; algorithm in SURVEY.md sec. A).
//
// Why radix 2^29 (measured on MI355X, tools/microbench/valu_rates.hip,
// profiles/r01_valu_rates.txt): v_mad_u64_u32 issues at the same ~4 cycles per
// wave64 as a 32-bit add-with-carry, so the cheapest 254-bit multiplier is the one
// with the fewest instructions of any kind.  Nine 29-bit limbs leave 6 spare bits in
// a 64-bit column accumulator: up to 36 limb products (58 bits each) are summed with
// one v_mad_u64_u32 apiece and NO carry instructions; the carry is taken once per
// column (v_lshrrev_b64 + v_and).  A Montgomery product is 81 + 81 mads + 9 mul_lo +
// ~34 shifts/ands instead of 128 mads + 128 carry ops with 32-bit limbs.  FP64-FMA
// limbs (5.2 cycles per v_fma_f64, 2 FMAs + 1 add + 2 integer adds per limb product)
// and 24-bit multiplies were measured slower.
//
// Value domain: Montgomery with R = 2^261.  Stored field elements (HBM, API buffers in
// device format) are fully reduced (< p) and packed as 8 x u32 little-endian.
#pragma once
#include <cstddef>
#include <cstdint>
#include "imt_consts.hpp"

// The arithmetic below is plain integer C++, so tests/native/ can also compile it for the
// host (g++) and check it against the oracle without a GPU.  Under hipcc everything is
// force-inlined device code.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define IMT_HD __host__ __device__ __forceinline__
#else
#define IMT_HD inline
#endif

namespace imt {
namespace dev {

// p = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001 in 29-bit limbs
#define IMT_P29_0 0x10000001u
#define IMT_P29_1 0x1f0fac9fu
#define IMT_P29_2 0x0e5c2450u
#define IMT_P29_3 0x07d090f3u
#define IMT_P29_4 0x1585d283u
#define IMT_P29_5 0x02db40c0u
#define IMT_P29_6 0x00a6e141u
#define IMT_P29_7 0x0e5c2634u
#define IMT_P29_8 0x0030644eu
constexpr uint32_t N0INV29 = 0x0fffffffu;   // -p^-1 mod 2^29
constexpr uint32_t N0INV32 = 0xefffffffu;   // -p^-1 mod 2^32

IMT_HD constexpr uint32_t p29(int i) {
    return i == 0 ? IMT_P29_0 : i == 1 ? IMT_P29_1 : i == 2 ? IMT_P29_2 : i == 3 ? IMT_P29_3 :
           i == 4 ? IMT_P29_4 : i == 5 ? IMT_P29_5 : i == 6 ? IMT_P29_6 : i == 7 ? IMT_P29_7 : IMT_P29_8;
}


// ---------------------------------------------------------------------------------
// Montgomery reduction of a sum of NT limb products plus (optionally) addend * R.
//   r = (sum_t a[t]*b[t] + addend*R + m*p) / R
// The quotient digits m_k only have to clear the low 29 bits of their column.  With WIDE_M they
// are taken as full 32-bit words, m_k = lo32(column) * (-p^-1 mod 2^32), which saves the mask per
// digit; the column then has its low 32 bits clear and the result grows by up to 8p instead of p
// (m < 2^264 = 8R):
//   WIDE_M : r < sum/R + addend + 8p        !WIDE_M : r < sum/R + addend + p
// Column accumulators must stay below 2^64.  A column holds each limb of p at most once, so its
// m*p part is below 2^32 * (sum of the limbs of p) = 0.4251 * 2^64 (WIDE_M) or 9 * 2^58 (!WIDE_M);
// the a*b part is at most NT * 9 * max(a limb) * max(b limb), and the carry-in is below 2^36:
//   NT = 4, 29-bit limbs : 36 * 2^58 = 0.5625 * 2^64   -> 0.9876 * 2^64 with WIDE_M
//   NT = 1, 30-bit limbs on both sides : 9 * 2^60 = 0.5625 * 2^64 -> the same
// Output limbs are normalised (< 2^29; the top limb holds whatever is left, so values must stay
// below 2^261 = 169p: every lane that is only ever ADDED to between multiplications -- the linear
// lanes of the partial rounds -- uses !WIDE_M).
// ---------------------------------------------------------------------------------
template <bool WIDE_M>
IMT_HD uint32_t mont_digit(uint64_t acc) {
    return WIDE_M ? (uint32_t)acc * N0INV32 : (((uint32_t)acc * N0INV29) & MASK29);
}

}  // namespace dev
}  // namespace imt
// On the device the products below are replaced by hand-laid single-chain assembly with the same
// values (generated; see tools/gen_mont_asm.py).  -DIMT_NO_MONT_ASM keeps the C++ forms.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(IMT_NO_MONT_ASM)
#define IMT_MONT_ASM 1
#include "imt_mont_asm.hpp"
#include "imt_mont_asm_rec.hpp"
#endif
namespace imt {
namespace dev {

template <int NT, bool ADD, bool WIDE_M = true>
IMT_HD void mont_dot(Fe& r, const Fe* a, const Fe* b, const Fe& addend) {
    uint32_t m[NL];
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < NL; k++) {
#pragma unroll
        for (int t = 0; t < NT; t++) {
#pragma unroll
            for (int i = 0; i <= k; i++) acc += (uint64_t)a[t].v[i] * b[t].v[k - i];
        }
#pragma unroll
        for (int i = 0; i < k; i++) acc += (uint64_t)m[i] * p29(k - i);
        m[k] = mont_digit<WIDE_M>(acc);
        acc += (uint64_t)m[k] * p29(0);
        acc >>= 29;
    }
#pragma unroll
    for (int k = NL; k < 2 * NL - 1; k++) {
#pragma unroll
        for (int t = 0; t < NT; t++) {
#pragma unroll
            for (int i = k - (NL - 1); i < NL; i++) acc += (uint64_t)a[t].v[i] * b[t].v[k - i];
        }
#pragma unroll
        for (int i = k - (NL - 1); i < NL; i++) acc += (uint64_t)m[i] * p29(k - i);
        if (ADD) acc += addend.v[k - NL];
        r.v[k - NL] = (uint32_t)acc & MASK29;
        acc >>= 29;
    }
    if (ADD) acc += addend.v[NL - 1];
    r.v[NL - 1] = (uint32_t)acc;
}

IMT_HD void mont_mul(Fe& r, const Fe& a, const Fe& b) {
#ifdef IMT_MONT_ASM
    masm::mul_vv(r, &a, &b);
#else
    mont_dot<1, false>(r, &a, &b, a);
#endif
}

// mont_dot whose first factors `c` are wave-uniform constants (entries of the __constant__ Poseidon
// tables indexed by the round counter).  Only permute() may use it: see imt_mont_asm.hpp.
template <int NT, bool ADD, bool WIDE_M = true>
IMT_HD void mont_dot_uc(Fe& r, const Fe* c, const Fe* v, const Fe& addend) {
#ifdef IMT_MONT_ASM
    static_assert((NT == 3 && !ADD && WIDE_M) || (NT == 4 && WIDE_M) || (NT == 2 && ADD && !WIDE_M),
                  "no assembly form for this shape");
    if constexpr (NT == 3) masm::dot3_uc(r, c, v);
    else if constexpr (NT == 4 && ADD) masm::dot4_add_uc(r, c, v, addend);
    else if constexpr (NT == 4) masm::dot4_uc(r, c, v);
    else masm::dot2_add_uc_narrow(r, c, v, addend);
#else
    mont_dot<NT, ADD, WIDE_M>(r, c, v, addend);
#endif
}

// r = a^2 / R (+ up to 8p: wide quotient digits).  36 doubled cross products + 9 squares instead
// of 81 products.  Precondition: limbs of a < 2^30 (column 8: 4 * 2^31 * 2^30 + 2^60 = 0.5625 * 2^64).
IMT_HD void mont_sqr(Fe& r, const Fe& a) {
#ifdef IMT_MONT_ASM
    masm::sqr_v(r, a);
    return;
#endif
    uint32_t m[NL], a2[NL];
#pragma unroll
    for (int i = 0; i < NL; i++) a2[i] = a.v[i] << 1;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < NL; k++) {
#pragma unroll
        for (int i = 0; 2 * i < k; i++) acc += (uint64_t)a2[i] * a.v[k - i];
        if ((k & 1) == 0) acc += (uint64_t)a.v[k / 2] * a.v[k / 2];
#pragma unroll
        for (int i = 0; i < k; i++) acc += (uint64_t)m[i] * p29(k - i);
        m[k] = mont_digit<true>(acc);
        acc += (uint64_t)m[k] * p29(0);
        acc >>= 29;
    }
#pragma unroll
    for (int k = NL; k < 2 * NL - 1; k++) {
#pragma unroll
        for (int i = k - (NL - 1); 2 * i < k; i++) acc += (uint64_t)a2[i] * a.v[k - i];
        if ((k & 1) == 0) acc += (uint64_t)a.v[k / 2] * a.v[k / 2];
#pragma unroll
        for (int i = k - (NL - 1); i < NL; i++) acc += (uint64_t)m[i] * p29(k - i);
        r.v[k - NL] = (uint32_t)acc & MASK29;
        acc >>= 29;
    }
    r.v[NL - 1] = (uint32_t)acc;
}

// limb-wise add without carry propagation (limbs grow by one bit)
// r = a / R mod p (+ < p): out of the Montgomery domain without the 81 limb products of a multiplication by 1.
// a: normalised limbs (29-bit digits).  Same column structure as mont_dot with the value in the low nine columns.
IMT_HD void mont_redc(Fe& r, const Fe& a) {
    uint32_t m[NL];
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < NL; k++) {
        acc += a.v[k];
#pragma unroll
        for (int i = 0; i < k; i++) acc += (uint64_t)m[i] * p29(k - i);
        m[k] = mont_digit<false>(acc);
        acc += (uint64_t)m[k] * p29(0);
        acc >>= 29;
    }
#pragma unroll
    for (int k = NL; k < 2 * NL - 1; k++) {
#pragma unroll
        for (int i = k - (NL - 1); i < NL; i++) acc += (uint64_t)m[i] * p29(k - i);
        r.v[k - NL] = (uint32_t)acc & MASK29;
        acc >>= 29;
    }
    r.v[NL - 1] = (uint32_t)acc;
}

IMT_HD void add_lazy(Fe& r, const Fe& a, const Fe& b) {
#pragma unroll
    for (int i = 0; i < NL; i++) r.v[i] = a.v[i] + b.v[i];
}

IMT_HD void normalize(Fe& a) {
#pragma unroll
    for (int i = 0; i < NL - 1; i++) {
        a.v[i + 1] += a.v[i] >> 29;
        a.v[i] &= MASK29;
    }
}

// a >= p ?  (normalised limbs)
IMT_HD bool geq_p(const Fe& a) {
    bool ge = true;   // equal so far => >=
#pragma unroll
    for (int i = 0; i < NL; i++) {   // from least significant: later limbs override
        uint32_t pi = p29(i);
        if (a.v[i] != pi) ge = a.v[i] > pi;
    }
    return ge;
}

IMT_HD void sub_p(Fe& a) {
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        uint32_t d = a.v[i] - p29(i) - borrow;
        borrow = (i < NL - 1) ? (d >> 31) : 0;        // limbs < 2^29: bit 31 set <=> negative
        a.v[i] = (i < NL - 1) ? (d & MASK29) : d;
    }
}

// limb i of (p << SH), SH = 0..4
template <int SH>
IMT_HD constexpr uint32_t p29_shl(int i) {
    return i == 0 ? ((p29(0) << SH) & MASK29)
         : i < NL - 1 ? (((p29(i) << SH) | (p29(i - 1) >> (29 - SH))) & MASK29)
                      : ((p29(i) << SH) | (p29(i - 1) >> (29 - SH)));
}
// a -= (p << SH) if a >= (p << SH)   (normalised limbs)
template <int SH>
IMT_HD void cond_sub_p_shl(Fe& a) {
    bool ge = true;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const uint32_t pi = p29_shl<SH>(i);
        if (a.v[i] != pi) ge = a.v[i] > pi;
    }
    if (ge) {
        uint32_t borrow = 0;
#pragma unroll
        for (int i = 0; i < NL; i++) {
            uint32_t d = a.v[i] - p29_shl<SH>(i) - borrow;
            borrow = (i < NL - 1) ? (d >> 31) : 0;
            a.v[i] = (i < NL - 1) ? (d & MASK29) : d;
        }
    }
}

// bring a normalised value < 32p into [0, p)
IMT_HD void canonicalize(Fe& a) {
    cond_sub_p_shl<4>(a);
    cond_sub_p_shl<3>(a);
    cond_sub_p_shl<2>(a);
    cond_sub_p_shl<1>(a);
    cond_sub_p_shl<0>(a);
}

// 8 x u32 packed (value < 2^256) <-> 9 x 29-bit limbs
IMT_HD void unpack(Fe& r, const uint32_t w[8]) {
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const int bit = 29 * i, wi = bit >> 5, sh = bit & 31;
        uint32_t lo = w[wi] >> sh;
        if (sh > 3 && wi + 1 < 8) lo |= w[wi + 1] << (32 - sh);
        r.v[i] = lo & MASK29;
    }
}
IMT_HD void pack(uint32_t w[8], const Fe& a) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        // word j covers bits [32j, 32j+32)
        const int lo_limb = (32 * j) / 29, off = 32 * j - 29 * lo_limb;
        uint32_t x = a.v[lo_limb] >> off;
        const int have = 29 - off;
        if (have < 32 && lo_limb + 1 < NL) x |= a.v[lo_limb + 1] << have;
        if (have + 29 < 32 && lo_limb + 2 < NL) x |= a.v[lo_limb + 2] << (have + 29);
        w[j] = x;
    }
}

struct alignas(16) Word4 { uint32_t x, y, z, w; };   // one 16-byte global access
IMT_HD void load_packed(Fe& r, const void* ptr) {
    const Word4* q = reinterpret_cast<const Word4*>(ptr);
    Word4 x = q[0], y = q[1];
    uint32_t w[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
    unpack(r, w);
}
IMT_HD void store_packed(void* ptr, const Fe& a) {
    uint32_t w[8];
    pack(w, a);
    Word4* q = reinterpret_cast<Word4*>(ptr);
    q[0] = Word4{w[0], w[1], w[2], w[3]};
    q[1] = Word4{w[4], w[5], w[6], w[7]};
}

// ---------------------------------------------------------------------------------
// Constant tables (filled by the host from the Grain LFSR; imt_params.cpp).  All
// lanes of a wave read the same entry at the same time, so these are scalar loads.
// ---------------------------------------------------------------------------------


IMT_HD void sbox(Fe& x) {   // x <- x^5; limbs of x < 2^30
    Fe x2, x4;
    mont_sqr(x2, x);
    mont_sqr(x4, x2);
    mont_mul(x, x4, x);
}

// limb i of 2^261 - p (p's lowest limb is odd: no borrow past limb 0)
IMT_HD constexpr uint32_t pc29(int i) { return i == 0 ? (1u << 29) - p29(0) : MASK29 - p29(i); }
constexpr uint32_t FOLD_RECIP = 1354;   // floor(2^264 / p)

// a - q p with q = floor(top * floor(2^264/p) / 2^32) <= a / p: brings a lane that is only ever added to back
// below 1.2p.  a: normalised limbs, a < 2^261.  Computed as a + q (2^261 - p) - q 2^261 (nine mads, no borrows).
IMT_HD void fold_p(Fe& a) {
    const uint32_t q = (uint32_t)(((uint64_t)a.v[NL - 1] * FOLD_RECIP) >> 32);
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        acc = (acc >> 29) + a.v[i] + (uint64_t)q * pc29(i);
        a.v[i] = i < NL - 1 ? (uint32_t)acc & MASK29 : (uint32_t)(acc - ((uint64_t)q << 29));
    }
}

// One permutation, optimised schedule (same values as the plain 65-round form; tables from imt_params.cpp).
//   full rounds f = 0..3, 4..7 : lanes rescaled by fifth roots of constants, so that every S-box output arrives
//                                pre-multiplied by the factor the linear layer would apply to it: s += c_f; x^5 on all
//                                lanes; n = M_f s.  Row 0 of M_f is (1, 1, 1), i.e. a sum, except in f = 0 (the
//                                caller's unscaled input) and f = 4 (the partial rounds' exit)
//   partial rounds r = 0..56   : an order-3 recurrence on the S-box lane alone (Cayley-Hamilton on the MDS):
//                                z_r = (w_r + k_r)^5;  w_r+1 = c_r . (w_r, w_r-1, z_r-2, z_r-1) + z_r
// The S-box input is held rescaled so that z_r enters with coefficient 1, as the REDC addend: 4 products + 1 reduction
// per round besides the S-box.  Full round 3 seeds the window: its row 0 is w_0, its rows 1 and 2 the two functionals
// of lanes 1, 2 that w_1 = row 1 + z_0 and w_2 = c_1 . (w_1, z_0) + row 2 + z_1 need.  After round 56 lane 0 is w_57
// and lanes 1, 2 are rebuilt from (w_57, w_56, z_55, z_56) at the start of full round 4 (one dot3 call, taken twice).
// The window values are normalised REDC outputs (limbs < 2^29: the column budget of the 4-term form); only the S-box
// input is a lazy sum.
// One flat loop, one step per round, so that each body exists once in the instruction stream.  Kept flat on purpose:
// with the partial rounds as an inner loop of one step, the full rounds' block alone needed 93 VGPRs (75 flat) and the
// kernels capped at 96 spilled.  Flat, the window costs one extra lane (z3) carried through the full rounds.
// `first_rc` replaces the round-0 constants (sponge padding folded in by the caller); the input and the output
// are unscaled.  Entry: limbs normalised, lane 0 < 32p, lanes 1, 2 < 16p.  Exit: limbs normalised, lane 0
// < 30p (a sum of three S-box outputs), lanes 1, 2 < 9p.  Bounds: tests/test_recurrence_schedule_bounds.py.
IMT_HD void permute(const PoseidonConsts& pc, Fe s[3], const Fe* first_rc) {
    constexpr int NSTEP = RF + RP;             // 4 full rounds, 57 partial rounds, 4 full rounds
    // partial round r: s[0] = w_r, s[1] = w_r-1, z3 = z_r-2, s[2] = z_r-1 (rounds 0, 1: the seeds)
    Fe z3;
#pragma unroll
    for (int i = 0; i < NL; i++) z3.v[i] = 0;
#pragma unroll 1
    for (int st = 0; st < NSTEP; st++) {
        if (st < RF / 2 || st >= RF / 2 + RP) {
            const int fr = st < RF / 2 ? st : st - RP;
            if (fr == RF / 2) {
                // lanes 1, 2 of full round 4's input: rec_exit[i] . (w_57, w_56, z_55) + z_56
                const Fe v[3] = {s[0], s[1], z3};
                const Fe zl = s[2];
#pragma unroll 1
                for (int i = 0; i < 2; i++) {
                    Fe n;
                    mont_dot_uc<3, false>(n, pc.rec_exit[i], v, v[0]);
                    add_lazy(n, n, zl);
                    normalize(n);
                    s[1] = s[2]; s[2] = n;
                }
            }
            const Fe* rc = (st == 0) ? first_rc : pc.sc_rc[fr];
            add_lazy(s[0], s[0], rc[0]);
            add_lazy(s[1], s[1], rc[1]);
            add_lazy(s[2], s[2], rc[2]);
            sbox(s[0]); sbox(s[1]); sbox(s[2]);
            const Fe(*mat)[3] = pc.sc_mats[fr];
            Fe n0, n1, n2;
            if (fr == 0 || fr == RF / 2) {
                mont_dot_uc<3, false>(n0, mat[0], s, s[0]);
            } else {
                add_lazy(n0, s[0], s[1]);
                add_lazy(n0, n0, s[2]);
                normalize(n0);
            }
            mont_dot_uc<3, false>(n1, mat[1], s, s[0]);
            mont_dot_uc<3, false>(n2, mat[2], s, s[0]);
            s[0] = n0; s[1] = n1; s[2] = n2;
        } else {
            const int r = st - RF / 2;
            Fe z, w;
            add_lazy(z, s[0], pc.rec_k[r]);
            sbox(z);
            if (r >= 2) {
                const Fe v[4] = {s[0], s[1], z3, s[2]};
                mont_dot_uc<4, true>(w, pc.rec_c[r], v, z);
            } else if (r == 1) {                       // w_2 = c . (w_1, z_0) + L2 + z_1
                const Fe v[2] = {s[0], s[2]};
                Fe e;
                add_lazy(e, z3, z);
                mont_dot_uc<2, true, false>(w, pc.rec_c[1], v, e);
            } else {                                   // w_1 = L1 + z_0
                add_lazy(w, s[1], z);
                normalize(w);
            }
            s[1] = s[0]; s[0] = w; z3 = s[2]; s[2] = z;
        }
    }
}

// Poseidon::update(&[a,b]) or update(&[a,b,c]) followed by squeeze_and_reset():
// two permutations either way.  `three` must be wave-uniform.
IMT_HD void hash23(const PoseidonConsts& pc, Fe& out, const Fe& a, const Fe& b, const Fe& c, bool three) {
    Fe s[3] = {pc.cap0, a, b};
#pragma unroll 1
    for (int blk = 0; blk < 2; blk++) {
        const Fe* rc0 = pc.rc_full[0];
        if (blk == 1) {
            if (three) {               // absorb [c, 1] into lanes 1, 2
                add_lazy(s[1], s[1], c);
                add_lazy(s[2], s[2], pc.one);
                normalize(s[1]);
                normalize(s[2]);
            } else {                   // absorb the padding 1 into lane 1 (folded into rc)
                rc0 = pc.rc_h2p2;
            }
        }
        permute(pc, s, rc0);
    }
    out = s[1];
    canonicalize(out);
}
// The same with the third input parked in a per-thread slot of `stash` (LDS on the device: stash[limb * stride]),
// written by the caller and read back only where the second permutation absorbs it: nine registers fewer are live
// across the first permutation, which is what lets ONE copy of the hash serve 2- and 3-input callers at 96 VGPRs.
IMT_HD void hash23_stashed(const PoseidonConsts& pc, Fe& out, const Fe& a, const Fe& b, bool three,
                           const uint32_t* stash, unsigned stride) {
    Fe s[3] = {pc.cap0, a, b};
#pragma unroll 1
    for (int blk = 0; blk < 2; blk++) {
        const Fe* rc0 = pc.rc_full[0];
        if (blk == 1) {
            if (three) {               // absorb [c, 1] into lanes 1, 2
                Fe c;
#pragma unroll
                for (int i = 0; i < NL; i++) c.v[i] = stash[(size_t)i * stride];
                add_lazy(s[1], s[1], c);
                add_lazy(s[2], s[2], pc.one);
                normalize(s[1]);
                normalize(s[2]);
            } else {                   // absorb the padding 1 into lane 1 (folded into rc)
                rc0 = pc.rc_h2p2;
            }
        }
        permute(pc, s, rc0);
    }
    out = s[1];
    canonicalize(out);
}
// Poseidon::update(&in[0 .. len]) followed by squeeze_and_reset() for any len >= 1 -- halo2-base's hash_fix_len_array over
// a slice of the caller's choosing: floor(len / 2) + 1 permutations.  Every full pair of inputs goes into lanes 1, 2; the
// last permutation takes the leftover input (len odd) and the padding 1 in the next free lane(s).  One loop around ONE
// permute(), the inputs of a chunk fetched inside it by `load(j, x)` (input j of this hash, canonical device form), so
// that no more than one input is ever held beside the state.  Absorbing is hash23's `three` branch: lanes 1, 2 leave
// permute() below 9p, an input is below p, so they enter the next one below 10p (entry bound 16p); lane 0 is untouched
// (< 30p, bound 32p).  For len even the padding rides on the round-0 constants (rc_h2p2).  `len` must be wave-uniform.
// len = 2, 3 give hash23's values limb for limb.
template <class LoadInput>
IMT_HD void hash_sponge(const PoseidonConsts& pc, Fe& out, unsigned len, LoadInput load) {
    Fe s[3];
    s[0] = pc.cap0;
#pragma unroll
    for (int i = 0; i < NL; i++) s[1].v[i] = s[2].v[i] = 0;     // PoseidonState::default: [2^64, 0, 0]
    const unsigned full = len >> 1;
#pragma unroll 1
    for (unsigned ch = 0; ch <= full; ch++) {
        const Fe* rc0 = pc.rc_full[0];
        if (ch < full || (len & 1u)) {
            Fe x;
            load(2 * ch, x);
            add_lazy(s[1], s[1], x);
            normalize(s[1]);
            if (ch < full) load(2 * ch + 1, x);
            else x = pc.one;                                    // the padding behind the leftover input
            add_lazy(s[2], s[2], x);
            normalize(s[2]);
        } else {                       // nothing left but the padding 1 in lane 1 (folded into rc)
            rc0 = pc.rc_h2p2;
        }
        permute(pc, s, rc0);
    }
    out = s[1];
    canonicalize(out);
}
IMT_HD void hash2(const PoseidonConsts& pc, Fe& out, const Fe& a, const Fe& b) { hash23(pc, out, a, b, a, false); }
IMT_HD void hash3(const PoseidonConsts& pc, Fe& out, const Fe& a, const Fe& b, const Fe& c) { hash23(pc, out, a, b, c, true); }

// ---- boundary formats ----------------------------------------------------------
enum : unsigned { FMT_CANONICAL = 0, FMT_MONT256 = 1, FMT_DEVICE = 2 };

// returns false if the stored integer is >= p (canonical / mont256 inputs must be reduced)
IMT_HD bool load_fe(const PoseidonConsts& pc, Fe& r, const void* ptr, unsigned fmt) {
    Fe raw;
    load_packed(raw, ptr);
    bool ok = !geq_p(raw) && (raw.v[NL - 1] >> 24) == 0;   // top limb holds bits 232..255
    if (fmt == FMT_DEVICE) { r = raw; return ok; }
    mont_mul(r, raw, fmt == FMT_CANONICAL ? pc.from_canon : pc.from_mont256);
    canonicalize(r);
    return ok;
}
IMT_HD void store_fe(const PoseidonConsts& pc, void* ptr, const Fe& a, unsigned fmt) {
    if (fmt == FMT_DEVICE) { store_packed(ptr, a); return; }
    Fe t;
    mont_mul(t, a, fmt == FMT_CANONICAL ? pc.int_one : pc.to_mont256);
    canonicalize(t);
    store_packed(ptr, t);
}

IMT_HD bool fe_eq(const Fe& a, const Fe& b) {   // both canonical
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) d |= a.v[i] ^ b.v[i];
    return d == 0;
}
IMT_HD bool fe_is_zero(const Fe& a) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) d |= a.v[i];
    return d == 0;
}

}  // namespace dev
}  // namespace imt
