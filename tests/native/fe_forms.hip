// fe_forms.hip -- TEST-ONLY gfx950 harness: the inline-assembly Montgomery forms of csrc/imt_mont_asm.hpp, the device
// helpers they feed and both permutation schedules, on raw limbs with no canonical check, so that
// tests/test_gpu_fe_forms.py can compare them with tests/fe_model.py bit for bit as integers (not mod p).
// Not part of libimt_hip.so; tests/test_gpu_fe_forms.py builds it (hipcc -shared) and calls it through ctypes.
#include <hip/hip_runtime.h>
#include <cstring>
#include <string>
#include "imt_device.hpp"
#include "imt_trace_device.hpp"
#include "imt_params.hpp"
// the assembly forms and the coop schedule exist only in the device pass; the host pass sees empty kernel bodies
#if defined(__HIP_DEVICE_COMPILE__)
#include "imt_coop_device.hpp"
#define DEVICE_ONLY(...) __VA_ARGS__
#else
#define DEVICE_ONLY(...)
#endif

using namespace imt;
using namespace imt::dev;

__constant__ PoseidonConsts c_pc;

constexpr unsigned BLOCK = 64;     // one wave per block: neighbouring waves of a launch take different constants

__device__ __forceinline__ void ld(Fe& r, const uint32_t* p) {
#pragma unroll
    for (int i = 0; i < NL; i++) r.v[i] = p[i];
}
__device__ __forceinline__ void st(uint32_t* p, const Fe& r) {
#pragma unroll
    for (int i = 0; i < NL; i++) p[i] = r.v[i];
}

// ---- one kernel per assembly form ------------------------------------------------------------------------------------
// in: [n][LANE_SLOTS][9], the per-lane operand slots in call order; uni: [gridDim.x][UNI_SLOTS][9], the uniform slots,
// one set per block (a scalar load: the real kernels index their tables by the round counter the same way).
#define FE_FORM(NAME, LANE_SLOTS, UNI_SLOTS, ...)                                                                   \
    extern "C" __global__ void __launch_bounds__(BLOCK)                                                            \
    fek_##NAME(const uint32_t* __restrict__ in, const uint32_t* __restrict__ uni, uint32_t* __restrict__ out,       \
               unsigned n) {                                                                                        \
        const unsigned j = blockIdx.x * BLOCK + threadIdx.x;                                                        \
        if (j >= n) return;                                                                                         \
        Fe x[LANE_SLOTS + 1], u[UNI_SLOTS + 1], r = {};                                                             \
        _Pragma("unroll") for (int s = 0; s < LANE_SLOTS; s++) ld(x[s], in + (j * (LANE_SLOTS) + s) * NL);          \
        _Pragma("unroll") for (int s = 0; s < UNI_SLOTS; s++) ld(u[s], uni + (blockIdx.x * (UNI_SLOTS) + s) * NL);  \
        DEVICE_ONLY(__VA_ARGS__);                                                                                   \
        st(out + j * NL, r);                                                                                        \
    }

FE_FORM(mul_vv, 2, 0, masm::mul_vv(r, &x[0], &x[1]))
FE_FORM(sqr_v, 1, 0, masm::sqr_v(r, x[0]))
FE_FORM(dot3_uc, 3, 3, masm::dot3_uc(r, u, x))
FE_FORM(dot4_uc, 4, 4, masm::dot4_uc(r, u, x))
FE_FORM(dot2_add_uc_narrow, 3, 2, masm::dot2_add_uc_narrow(r, u, x, x[2]))
FE_FORM(sqr_v_narrow, 1, 0, masm::sqr_v_narrow(r, x[0]))
FE_FORM(mul_vv_adds_narrow, 2, 1, masm::mul_vv_adds_narrow(r, &x[0], &x[1], u[0]))
FE_FORM(mul_uc_narrow, 1, 1, masm::mul_uc_narrow(r, &u[0], &x[0]))
FE_FORM(mul_uc_add_narrow, 2, 1, masm::mul_uc_add_narrow(r, &u[0], &x[0], x[1]))
FE_FORM(redc_v_narrow, 1, 0, masm::redc_v_narrow(r, x[0]))
FE_FORM(mul_vv_narrow, 2, 0, masm::mul_vv_narrow(r, &x[0], &x[1]))
FE_FORM(mul_vv_add_narrow, 3, 0, masm::mul_vv_add_narrow(r, &x[0], &x[1], x[2]))
FE_FORM(dot3_vv_narrow, 6, 0, {
    const Fe a[3] = {x[0], x[2], x[4]}, b[3] = {x[1], x[3], x[5]};
    masm::dot3_vv_narrow(r, a, b);
})

// ---- the helpers, on raw limbs / words: in [n][IW], out [n][OW] ---------------------------------------------------------
#define FE_HELPER(NAME, IW, OW, ...)                                                                                \
    extern "C" __global__ void __launch_bounds__(BLOCK)                                                            \
    feh_##NAME(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, unsigned n) {                           \
        const unsigned j = blockIdx.x * BLOCK + threadIdx.x;                                                        \
        if (j >= n) return;                                                                                         \
        const uint32_t* I = in + j * (IW);                                                                          \
        uint32_t* O = out + j * (OW);                                                                               \
        __VA_ARGS__;                                                                                                \
    }
#define FE_UNARY(NAME, CALL) FE_HELPER(NAME, NL, NL, { Fe a; ld(a, I); CALL(a); st(O, a); })

FE_UNARY(canonicalize, canonicalize)
FE_UNARY(fold_p, fold_p)
FE_UNARY(normalize, normalize)
FE_UNARY(cond_sub_p_shl0, cond_sub_p_shl<0>)
FE_UNARY(cond_sub_p_shl1, cond_sub_p_shl<1>)
FE_UNARY(cond_sub_p_shl2, cond_sub_p_shl<2>)
FE_UNARY(cond_sub_p_shl3, cond_sub_p_shl<3>)
FE_UNARY(cond_sub_p_shl4, cond_sub_p_shl<4>)
FE_UNARY(csub0, csub<0>)
FE_UNARY(csub1, csub<1>)
FE_HELPER(t_add, 2 * NL, NL, { Fe a, b, r; ld(a, I); ld(b, I + NL); t_add(r, a, b); st(O, r); })
FE_HELPER(pack, NL, 8, { Fe a; ld(a, I); pack(O, a); })
FE_HELPER(unpack, 8, NL, { Fe r; unpack(r, I); st(O, r); })
// load_fe: the limbs and the validity flag; store_fe / store_mont256: the eight words written (16-byte aligned rows)
#define FE_LOAD(F) FE_HELPER(load_fe##F, 8, NL + 1, { Fe r; O[NL] = load_fe(c_pc, r, I, F) ? 1u : 0u; st(O, r); })
#define FE_STORE(F) FE_HELPER(store_fe##F, NL, 8, { Fe a; ld(a, I); store_fe(c_pc, O, a, F); })
FE_LOAD(0)
FE_LOAD(1)
FE_LOAD(2)
FE_STORE(0)
FE_STORE(1)
FE_STORE(2)
FE_HELPER(store_mont256, NL, 8, { Fe a; ld(a, I); store_mont256(O, a); })

// ---- one permutation from raw entry lanes [n][3][9]; out: the raw exit lanes before canonicalize ------------------------
extern "C" __global__ void __launch_bounds__(BLOCK) fep_thread(const uint32_t* __restrict__ in,
                                                               uint32_t* __restrict__ out, unsigned n) {
    const unsigned j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    Fe s[3];
#pragma unroll
    for (int l = 0; l < 3; l++) ld(s[l], in + (j * 3 + l) * NL);
    permute(c_pc, s, c_pc.rc_full[0]);
#pragma unroll
    for (int l = 0; l < 3; l++) st(out + (j * 3 + l) * NL, s[l]);
}
// quad form: lanes 0, 1, 2 of a quad hold the state lanes, lane 3 shadows lane 0 (as in k_hash_batch_coop)
extern "C" __global__ void __launch_bounds__(BLOCK) fep_quad(const uint32_t* __restrict__ in,
                                                             uint32_t* __restrict__ out, unsigned n) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ uint32_t tab[coop::TAB_DWORDS];
    coop::tab_fill(tab, c_pc);
    const unsigned t = blockIdx.x * BLOCK + threadIdx.x, j = t >> 2;
    if (j >= n) return;
    const unsigned role = t & 3u, ri = role == 3u ? 0u : role;
    Fe S;
    ld(S, in + (j * 3 + ri) * NL);
    coop::permute(tab, S, ri, IMT_COOP_E(rc_full));
    if (role != 3u) st(out + (j * 3 + ri) * NL, S);
#endif
}

// ---- host side --------------------------------------------------------------------------------------------------------
struct Entry { const char* name; const void* fn; };
#define E(K) {#K, (const void*)K}
static const Entry FORMS[] = {E(fek_mul_vv), E(fek_sqr_v), E(fek_dot3_uc), E(fek_dot4_uc), E(fek_dot2_add_uc_narrow),
                              E(fek_sqr_v_narrow), E(fek_mul_vv_adds_narrow), E(fek_mul_uc_narrow),
                              E(fek_mul_uc_add_narrow), E(fek_redc_v_narrow), E(fek_mul_vv_narrow),
                              E(fek_mul_vv_add_narrow), E(fek_dot3_vv_narrow)};
static const Entry HELPERS[] = {E(feh_canonicalize), E(feh_fold_p), E(feh_normalize), E(feh_cond_sub_p_shl0),
                                E(feh_cond_sub_p_shl1), E(feh_cond_sub_p_shl2), E(feh_cond_sub_p_shl3),
                                E(feh_cond_sub_p_shl4), E(feh_csub0), E(feh_csub1), E(feh_t_add), E(feh_pack),
                                E(feh_unpack), E(feh_load_fe0), E(feh_load_fe1), E(feh_load_fe2), E(feh_store_fe0),
                                E(feh_store_fe1), E(feh_store_fe2), E(feh_store_mont256)};
static const void* find(const Entry* t, size_t n, const char* name) {
    for (size_t i = 0; i < n; i++)
        if (std::strcmp(t[i].name, name) == 0) return t[i].fn;
    return nullptr;
}

extern "C" int fe_init(void) {
    static bool done = false;
    if (done) return 0;
    HostPoseidon* hp = new HostPoseidon();
    std::string err;
    if (!hp->init(err)) return -1;
    PoseidonConsts pc;
    hp->fill_consts(pc);
    if (hipMemcpyToSymbol(HIP_SYMBOL(c_pc), &pc, sizeof pc) != hipSuccess) return -2;
    done = true;
    return 0;
}

// Copies in, runs one launch of `grid` blocks of BLOCK threads, copies out.  Sizes in 32-bit words.
static int run(const void* fn, unsigned grid, int n_dev, const uint32_t** host_in, const size_t* in_words,
               uint32_t* host_out, size_t out_words, unsigned n) {
    if (!fn) return -3;
    void* dev[3] = {nullptr, nullptr, nullptr};
    int rc = 0;
    for (int i = 0; i < n_dev && rc == 0; i++)
        if (hipMalloc(&dev[i], (in_words[i] ? in_words[i] : 1) * 4) != hipSuccess ||
            hipMemcpy(dev[i], host_in[i], in_words[i] * 4, hipMemcpyHostToDevice) != hipSuccess) rc = -4;
    void* d_out = nullptr;
    if (rc == 0 && (hipMalloc(&d_out, out_words * 4) != hipSuccess || hipMemset(d_out, 0xff, out_words * 4) != hipSuccess))
        rc = -4;
    if (rc == 0 && grid > 0) {
        void* args[5];
        int k = 0;
        for (int i = 0; i < n_dev; i++) args[k++] = &dev[i];
        args[k++] = &d_out;
        args[k++] = &n;
        if (hipLaunchKernel(fn, dim3(grid), dim3(BLOCK), args, 0, 0) != hipSuccess) rc = -5;
        else if (hipDeviceSynchronize() != hipSuccess) rc = -6;
    }
    if (rc == 0 && hipMemcpy(host_out, d_out, out_words * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = -7;
    for (int i = 0; i < n_dev; i++) (void)hipFree(dev[i]);
    (void)hipFree(d_out);
    return rc;
}

// form: lanes [n][lane_slots][9]; uni: [ceil(n / 64)][uni_slots][9]; out [n][9]
extern "C" int fe_form(const char* name, const uint32_t* lanes, unsigned lane_slots, const uint32_t* uni,
                       unsigned uni_slots, uint32_t* out, unsigned n) {
    const std::string k = std::string("fek_") + name;
    const unsigned grid = (n + BLOCK - 1) / BLOCK;
    const uint32_t* in[2] = {lanes, uni};
    const size_t w[2] = {(size_t)n * lane_slots * NL, (size_t)grid * uni_slots * NL};
    return run(find(FORMS, sizeof FORMS / sizeof *FORMS, k.c_str()), grid, 2, in, w, out, (size_t)n * NL, n);
}
// helper: in [n][in_words], out [n][out_words]
extern "C" int fe_helper(const char* name, const uint32_t* in, unsigned in_words, uint32_t* out, unsigned out_words,
                         unsigned n) {
    const std::string k = std::string("feh_") + name;
    const uint32_t* ins[1] = {in};
    const size_t w[1] = {(size_t)n * in_words};
    return run(find(HELPERS, sizeof HELPERS / sizeof *HELPERS, k.c_str()), (n + BLOCK - 1) / BLOCK, 1, ins, w,
               out, (size_t)n * out_words, n);
}
// permutation: quad = 0 thread form, 1 quad form; in / out [n][3][9]
extern "C" int fe_permute(int quad, const uint32_t* in, uint32_t* out, unsigned n) {
    const uint32_t* ins[1] = {in};
    const size_t w[1] = {(size_t)n * 3 * NL};
    const unsigned threads = quad ? 4 * n : n;
    return run(quad ? (const void*)fep_quad : (const void*)fep_thread, (threads + BLOCK - 1) / BLOCK, 1, ins, w,
               out, (size_t)n * 3 * NL, n);
}
