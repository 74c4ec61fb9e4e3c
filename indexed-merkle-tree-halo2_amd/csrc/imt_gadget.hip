// imt_gadget.hip -- f3: every NEW advice value the reference's insert_leaf assigns OUTSIDE hash_fix_len_array
// (imt_less_than_trace_batch, imt_insert_gadget_trace_batch; the hashes' own cells are imt_trace_device.hpp).
//
//   is_less_than          /root/reference/src/indexed_merkle_tree.rs:98-125  (two range.is_less_than(.,.,128), two
//                         gate.is_equal, not x4, and x3, and, or)
//   verify_non_inclusion  :127-229   insert_leaf :231-314   select :33-45   dual_mux :47-63   compute_merkle_root :78-96
//
// Row order = the order in which halo2-base's GateChip / RangeChip assign Witness cells (halo2-lib v0.4.x,
// gates/flex_gate.rs, gates/range.rs; UNPINNED BY THE REFERENCE like the f1 trace: the crate is not vendored):
//   sub(a,b) [W a-b, b, 1, a]   mul / and [0, a, b, W ab]   mul_add [c, a, b, W ab+c]   not(a) = sub(1, a)
//   or(a,b) [W 1-b, 1, b, 1, b, a, W 1-b, W a+b-ab]         is_zero(a) [W z, a, W 1/a, 1, 0, a, W z, 0]
//   range.is_less_than(a, b, 128): [W 2^padded+a-b, b, 1, W 2^padded+a, -2^padded, 1, a], the k + 1 limbs of the first
//   cell with their running sums [W l0, W l1, 2^lb, W s1, ...], is_zero(top limb)         (k = ceil(128 / lookup_bits))
//
// Nothing here is a hash: integer work on 256-bit values (limbs, shifted differences, booleans), subtractions mod p and
// one modular inverse per is_equal (binary extended Euclid on canonical integers).  One thread per item; rows are
// written canonical, row-major [rows][n] (a wave's 64 stores of one row are contiguous) or item-major; the C entry
// converts to the caller's format afterwards.
//
// What one thread does for its item -- the 256-bit helpers, the row emitters, gadget::less_than_item and
// gadget::insert_gadget_item -- is imt_gadget_device.hpp, which also compiles for the host (tests/native/emul_gadget.cpp);
// the kernels below are the index computation and the call, launch:: the grids.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "imt_gadget.hpp"
#include "imt_gadget_device.hpp"

namespace imt {
namespace {

constexpr int BLOCK = 128;

__global__ void __launch_bounds__(BLOCK) k_less_than_trace(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, size_t n,
                                                           unsigned lb, uint8_t* __restrict__ trace, uint64_t row_stride,
                                                           uint64_t item_stride, uint8_t* __restrict__ lt_out) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t lt = gadget::less_than_item(a, b, i, lb, trace, row_stride, item_stride);
    if (lt_out) lt_out[i] = (uint8_t)lt;
}

__global__ void __launch_bounds__(BLOCK)
k_insert_gadget(const uint8_t* __restrict__ low_leaf, const uint64_t* __restrict__ low_index, const uint8_t* __restrict__ new_leaf,
                unsigned new_stride /*96: leaves; 32: bare values*/, const uint64_t* __restrict__ new_path_index,
                const uint8_t* __restrict__ is_largest, const uint8_t* __restrict__ pairs /*[chains][depth][n][2][32] canonical*/,
                unsigned depth, unsigned lb, size_t n, int whole_insert /*0: verify_non_inclusion alone (one chain)*/,
                uint8_t* __restrict__ trace, uint64_t row_stride, uint64_t item_stride) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    gadget::insert_gadget_item(low_leaf, low_index, new_leaf, new_stride, new_path_index, is_largest, pairs, depth, lb, n, i,
                               whole_insert, trace, row_stride, item_stride);
}

}  // namespace

namespace launch {

void less_than_trace(hipStream_t s, const uint8_t* a, const uint8_t* b, size_t n, unsigned lookup_bits, uint8_t* trace,
                     uint64_t row_stride, uint64_t item_stride, uint8_t* lt_out) {
    if (!n) return;
    hipLaunchKernelGGL(k_less_than_trace, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, a, b, n, lookup_bits, trace,
                       row_stride, item_stride, lt_out);
}

void insert_gadget(hipStream_t s, const uint8_t* low_leaf, const uint64_t* low_index, const uint8_t* new_leaf,
                   const uint64_t* new_path_index, const uint8_t* is_largest, const uint8_t* pairs, unsigned depth,
                   unsigned lookup_bits, size_t n, uint8_t* trace, uint64_t row_stride, uint64_t item_stride) {
    if (!n) return;
    hipLaunchKernelGGL(k_insert_gadget, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, low_leaf, low_index, new_leaf,
                       96u, new_path_index, is_largest, pairs, depth, lookup_bits, n, 1, trace, row_stride, item_stride);
}

void non_inclusion_gadget(hipStream_t s, const uint8_t* low_leaf, const uint64_t* low_index, const uint8_t* new_val,
                          const uint8_t* is_largest, const uint8_t* pairs, unsigned depth, unsigned lookup_bits, size_t n,
                          uint8_t* trace, uint64_t row_stride, uint64_t item_stride) {
    if (!n) return;
    hipLaunchKernelGGL(k_insert_gadget, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, low_leaf, low_index, new_val,
                       32u, low_index, is_largest, pairs, depth, lookup_bits, n, 0, trace, row_stride, item_stride);
}

}  // namespace launch
}  // namespace imt
