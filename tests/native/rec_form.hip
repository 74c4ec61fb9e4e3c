// rec_form.hip -- TEST-ONLY harness of the partial rounds' Montgomery form dot4_add_uc (csrc/imt_mont_asm_rec.hpp):
//   r = (sum_{t<4} u[t] x[t] + e R) / R, u wave-uniform constants, x and e per lane, wide quotient digits.
// The gfx950 kernel runs the generated assembly; rec_form_host runs the C++ form the host build uses
// (mont_dot<4, true, true>).  tests/test_rec_form.py and tests/test_gpu_rec_form.py compare both with a Python model
// bit for bit, as raw limbs.  The same file builds with g++ (host entry only) and with hipcc (both entries).
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <cstdint>
#include "imt_device.hpp"

using namespace imt::dev;

// lanes: [n][5][9] = x[0..3], e; uni: [ceil(n / 64)][4][9], one set of constants per 64 lanes; out: [n][9]
extern "C" void rec_form_host(const uint32_t* lanes, const uint32_t* uni, uint32_t* out, unsigned n) {
    for (unsigned j = 0; j < n; j++) {
        Fe x[5], u[4], r;
        for (int s = 0; s < 5; s++)
            for (int i = 0; i < NL; i++) x[s].v[i] = lanes[((size_t)j * 5 + s) * NL + i];
        for (int s = 0; s < 4; s++)
            for (int i = 0; i < NL; i++) u[s].v[i] = uni[((size_t)(j / 64) * 4 + s) * NL + i];
        mont_dot<4, true, true>(r, u, x, x[4]);
        for (int i = 0; i < NL; i++) out[(size_t)j * NL + i] = r.v[i];
    }
}

#if defined(__HIPCC__)
constexpr unsigned BLOCK = 64;   // one wave per block: the constants of a block are one uniform set

extern "C" __global__ void __launch_bounds__(BLOCK) rek_dot4_add_uc(const uint32_t* __restrict__ in,
                                                                    const uint32_t* __restrict__ uni,
                                                                    uint32_t* __restrict__ out, unsigned n) {
    const unsigned j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    Fe x[5], u[4], r = {};
#pragma unroll
    for (int s = 0; s < 5; s++)
#pragma unroll
        for (int i = 0; i < NL; i++) x[s].v[i] = in[((size_t)j * 5 + s) * NL + i];
#pragma unroll
    for (int s = 0; s < 4; s++)
#pragma unroll
        for (int i = 0; i < NL; i++) u[s].v[i] = uni[((size_t)blockIdx.x * 4 + s) * NL + i];
#if defined(__HIP_DEVICE_COMPILE__)
    masm::dot4_add_uc(r, u, x, x[4]);
#endif
#pragma unroll
    for (int i = 0; i < NL; i++) out[(size_t)j * NL + i] = r.v[i];
}

extern "C" int rec_form_gpu(const uint32_t* lanes, const uint32_t* uni, uint32_t* out, unsigned n) {
    const unsigned grid = (n + BLOCK - 1) / BLOCK;
    const size_t w_in = (size_t)n * 5 * NL, w_uni = (size_t)grid * 4 * NL, w_out = (size_t)n * NL;
    void *d_in = nullptr, *d_uni = nullptr, *d_out = nullptr;
    int rc = 0;
    if (hipMalloc(&d_in, w_in * 4) != hipSuccess || hipMalloc(&d_uni, w_uni * 4) != hipSuccess ||
        hipMalloc(&d_out, w_out * 4) != hipSuccess)
        rc = -1;
    if (rc == 0 && (hipMemcpy(d_in, lanes, w_in * 4, hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(d_uni, uni, w_uni * 4, hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemset(d_out, 0xff, w_out * 4) != hipSuccess))
        rc = -2;
    if (rc == 0) {
        void* args[4] = {&d_in, &d_uni, &d_out, &n};
        if (hipLaunchKernel((const void*)rek_dot4_add_uc, dim3(grid), dim3(BLOCK), args, 0, 0) != hipSuccess) rc = -3;
        else if (hipDeviceSynchronize() != hipSuccess) rc = -4;
    }
    if (rc == 0 && hipMemcpy(out, d_out, w_out * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = -5;
    (void)hipFree(d_in);
    (void)hipFree(d_uni);
    (void)hipFree(d_out);
    return rc;
}
#endif
