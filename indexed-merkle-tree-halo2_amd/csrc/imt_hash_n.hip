// imt_hash_n.hip -- the fixed-length Poseidon hash of 1 to 16 inputs (imt_hash_n_batch, imt_hash_n_trace_batch):
// halo2-base's hash_fix_len_array over a slice of the caller's choosing, the function
//   hasher.hash_fix_len_array(ctx, gate, &inp)   /root/reference/src/indexed_merkle_tree.rs:92,194,271-275,299-303
// calls with 2 and 3 inputs, for what else a circuit that embeds the chip hashes with the same hasher (a note
// commitment of four to six fields, a nullifier derived from a commitment and a key).
//
// A translation unit of its own, with its own copies of the two constant tables, so that the kernels of
// imt_kernels.hip -- the ones the tree and the benchmark run -- are compiled from exactly the input they had before.
// The stages are imt_device.hpp::hash_sponge, imt_coop_device.hpp::hash_sponge and
// imt_trace_device.hpp::hash_sponge_trace: one loop around one copy of the permutation, the inputs of a chunk loaded
// inside the loop from the item's [len][32] row.
#include <hip/hip_runtime.h>

#include "imt_device.hpp"
#include "imt_trace_device.hpp"
#include "imt_launch.hpp"
#if defined(__HIP_DEVICE_COMPILE__)
#include "imt_coop_device.hpp"
#endif

namespace imt {
namespace {
using namespace dev;

__constant__ PoseidonConsts g_hn_pc;
__constant__ TraceConsts g_hn_tc;

constexpr int BLOCK = 256;
// 5 waves per SIMD (96 VGPRs), as every hash kernel of imt_kernels.hip
#ifndef IMT_HASH_WAVES
#define IMT_HASH_WAVES __attribute__((amdgpu_waves_per_eu(5, 5)))
#endif

__device__ __forceinline__ size_t gtid() { return (size_t)blockIdx.x * blockDim.x + threadIdx.x; }
// recomputed where it is called: three instructions instead of two registers kept across the permutation
__device__ __forceinline__ size_t gtid_again() {
    uint32_t lo = blockIdx.x * blockDim.x + threadIdx.x, hi = (uint32_t)(((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 32);
    asm volatile("" : "+v"(lo), "+v"(hi));
    return ((size_t)hi << 32) | lo;
}
__device__ __forceinline__ void flag_err(int* err, bool ok) {
    if (!ok && err) atomicOr(err, 1);
}

// input j of item `item` of in[n][len][32]; item < n and j < len, so the element lies inside the caller's buffer
struct InputAt {
    const uint8_t* in;
    unsigned len, fmt_in;
    bool* ok;
    __device__ __forceinline__ void operator()(unsigned j, Fe& x) const {
        *ok &= load_fe(g_hn_pc, x, in + (gtid_again() * len + j) * 32, fmt_in);
    }
};

// one thread per hash
__global__ IMT_HASH_WAVES void __launch_bounds__(BLOCK) k_hash_n(const uint8_t* __restrict__ in, unsigned len,
                                                                  uint8_t* __restrict__ out, size_t n, unsigned fmt_in,
                                                                  unsigned fmt_out, int* err) {
    if (gtid() >= n) return;
    bool ok = true;
    Fe o;
    hash_sponge(g_hn_pc, o, len, InputAt{in, len, fmt_in, &ok});
    store_fe(g_hn_pc, out + gtid_again() * 32, o, fmt_out);
    flag_err(err, ok);
}

// the same for few hashes: a quad of lanes per hash (imt_coop_device.hpp)
__global__ IMT_HASH_WAVES void __launch_bounds__(BLOCK) k_hash_n_coop(const uint8_t* __restrict__ in, unsigned len,
                                                                       uint8_t* __restrict__ out, size_t n, unsigned fmt_in,
                                                                       unsigned fmt_out, int* err) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ uint32_t tab[coop::TAB_DWORDS];
    coop::tab_fill(tab, g_hn_pc);
    if ((gtid() >> 2) >= n) return;
    const unsigned role = threadIdx.x & 3u, ri = role == 3u ? 0u : role;
    bool ok = true;
    Fe o;
    // the item number is rebuilt at every load and at the store: no address is kept across the permutation
    coop::hash_sponge(tab, o, len, ri, [&](unsigned j, Fe& x) {
        ok &= load_fe(g_hn_pc, x, in + ((gtid_again() >> 2) * len + j) * 32, fmt_in);
    });
    if ((threadIdx.x & 3u) == 1u) store_fe(g_hn_pc, out + (gtid_again() >> 2) * 32, o, fmt_out);
    flag_err(err, ok);
#endif
}

// one thread per hash: rows(len) rows of 32 bytes, row-major [rows][n] (a wave's 64 stores of one row are 2 KiB
// contiguous) or item-major [n][rows].  No register cap, as k_hash_trace.
template <unsigned FMT_OUT>
__global__ void __launch_bounds__(BLOCK) k_hash_n_trace(const uint8_t* __restrict__ in, unsigned len, size_t n,
                                                        uint8_t* __restrict__ trace, size_t rows, int item_major,
                                                        unsigned fmt_in, int* err) {
    const size_t i = gtid();
    if (i >= n) return;
    const uint8_t* p = in + i * 32 * (size_t)len;
    bool ok = true;
    TraceSink o{item_major ? trace + i * rows * 32 : trace + i * 32, item_major ? (uint64_t)32 : (uint64_t)n * 32};
    hash_sponge_trace<FMT_OUT>(g_hn_pc, g_hn_tc, o, len,
                               [&](unsigned j, Fe& x) { ok &= load_fe(g_hn_pc, x, p + (size_t)j * 32, fmt_in); });
    flag_err(err, ok);
}

inline unsigned nblk(size_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

}  // namespace

namespace launch {

hipError_t upload_hash_n_consts(const dev::PoseidonConsts& pc, const dev::TraceConsts& tc) {
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_hn_pc), &pc, sizeof(pc), 0, hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_hn_tc), &tc, sizeof(tc), 0, hipMemcpyHostToDevice);
}
void hash_n_batch(hipStream_t s, const uint8_t* in, unsigned len, uint8_t* out, size_t n, unsigned fmt_in, unsigned fmt_out,
                  int* err, uint32_t coop_max) {
    if (!n) return;
    if (n * 4 <= coop_max)
        hipLaunchKernelGGL(k_hash_n_coop, dim3(nblk(n * 4)), dim3(BLOCK), 0, s, in, len, out, n, fmt_in, fmt_out, err);
    else
        hipLaunchKernelGGL(k_hash_n, dim3(nblk(n)), dim3(BLOCK), 0, s, in, len, out, n, fmt_in, fmt_out, err);
}
void hash_n_trace(hipStream_t s, const uint8_t* in, unsigned len, size_t n, uint8_t* trace, size_t rows, bool item_major,
                  unsigned fmt_in, unsigned fmt_out, int* err) {
    if (!n) return;
    auto* k = fmt_out == FMT_MONT256 ? k_hash_n_trace<FMT_MONT256>
              : fmt_out == FMT_DEVICE ? k_hash_n_trace<FMT_DEVICE> : k_hash_n_trace<FMT_CANONICAL>;
    hipLaunchKernelGGL(k, dim3(nblk(n)), dim3(BLOCK), 0, s, in, len, n, trace, rows, item_major ? 1 : 0, fmt_in, err);
}

}  // namespace launch
}  // namespace imt
