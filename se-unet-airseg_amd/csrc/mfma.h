// Matrix-instruction and fragment layer of the convolution kernels (conv_igemm, conv_stream, conv_march, wgrad, wgrad_stream,
// wgrad_march, wgrad_1x1): the one definition of the vector types, of the 16-bit MFMA dispatch, of the transposing fragment
// read with its swizzle and of the compile-time loop.  Internal, device code only.
//
// A 16-bit fragment is 8 x 16-bit PATTERNS per lane and is carried as bf16x8 whatever the storage type: the LDS reads (plain
// and transposing) are type-agnostic, and only the matrix instruction follows the storage type T (bf16_t | f16_t; for f16 the
// fragments are bit-cast, which costs no instruction).  v_mfma_f32_16x16x32 has two forms, and a kernel uses one of them: the
// builtin (mfma_16x16x32; the compiler schedules it and allocates the accumulator -- every kernel but one) and inline asm with
// the accumulator pinned to the accumulator half of the register file (mfma_16x16x32_pinned: wgrad_march.hip).
// The transposing read (ds_read_b64_tr_b16) delivers "4 voxels of one channel" per lane from a voxel-major LDS image: within a
// 16-lane group, lane i receives column i of the 4 rows x 16 columns that the group's 16 addresses (8 bytes each) cover; two
// reads make the 8-element K-slice of a 16x16x32 operand (frag_tr16).  The two kernels that read voxel-major records this way
// share tr16_swz; march_swz describes conv_march.hip's own layout (plain 16-byte reads) and stays there.
#pragma once
#include <hip/hip_runtime.h>
#include <utility>
#include <type_traits>
#include "seunet_common.h"

namespace seunet {

typedef bf16_t bf16x4 __attribute__((ext_vector_type(4)));
typedef bf16_t bf16x8 __attribute__((ext_vector_type(8)));
typedef f16_t f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

// c + a x b, 16x16 tile, K = 32 (8 per lane); T = the storage type of the fragments
template <typename T> __device__ __forceinline__ f32x4 mfma_16x16x32(bf16x8 a, bf16x8 b, f32x4 c) {
  if constexpr (std::is_same<T, f16_t>::value)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// c + a x b, 32x32 tile, K = 16
template <typename T> __device__ __forceinline__ f32x16 mfma_32x32x16(bf16x8 a, bf16x8 b, f32x16 c) {
  if constexpr (std::is_same<T, f16_t>::value)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// The matrix instruction as inline asm with the accumulator pinned to the accumulator half of the register file ("+a": D = C
// in place).  Through the builtin the register allocator spread the 216 accumulator registers over both halves and then
// spilled fragments; the asm leaves the vector half to the fragments and addresses.  Its operands are ordinary data
// dependencies (the compiler still waits for the LDS reads that produce them); an accumulator is only read back after the
// last march (behind explicit wait states).
template <typename T> __device__ __forceinline__ void mfma_16x16x32_pinned(f32x4& c, bf16x8 a, bf16x8 b) {
  if constexpr (std::is_same<T, f16_t>::value) asm("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
  else asm("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}

// one transposing read; two of them side by side: the 8 elements of a K-slice; the same from two LDS byte addresses
__device__ __forceinline__ bf16x4 read_tr16(const lds_bf16x4* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(const_cast<lds_bf16x4*>(p));
}
__device__ __forceinline__ bf16x8 frag_join(bf16x4 lo, bf16x4 hi) { return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7); }
__device__ __forceinline__ bf16x8 frag_tr16(const lds_bf16x4* p0, const lds_bf16x4* p1) { return frag_join(read_tr16(p0), read_tr16(p1)); }
__device__ __forceinline__ bf16x8 frag_tr16(unsigned addr0, unsigned addr1) {
  return frag_tr16((const lds_bf16x4*)(size_t)addr0, (const lds_bf16x4*)(size_t)addr1);
}

// Piece permutation for voxel-major records of np 16-byte pieces (np = 4, 8, 16: 64-, 128-, 256-byte records) that are read
// by frag_tr16, as wgrad_march.hip and wgrad_1x1.hip lay their planes out.  A transposing read takes, per 16 lanes, 4
// consecutive voxels x 32 bytes (two adjacent pieces); 32 lanes = the voxels v..v+3 and v+8..v+11.  64-byte records: the four
// voxels already sit in different banks, bit 3 of v separates the two groups.  128-byte records: voxels v and v+2 share their
// banks -> bit 1 of v moves the piece pair, bit 3 separates the groups.  256-byte records: all four voxels share them -> bits
// 0-1 move the pair.  The XOR acts on the pair index (bit 0 of the piece stays); it is applied on the DMA source side and on
// the read.
__device__ __forceinline__ int tr16_swz(int np, int v) {
  if (np == 4) return ((v >> 3) & 1) << 1;
  if (np == 8) return (((v >> 1) & 1) | (((v >> 3) & 1) << 1)) << 1;
  return ((v & 3) | (((v >> 3) & 1) << 2)) << 1;
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): the index is a constant expression inside f
template <int N, typename F> __device__ __forceinline__ void static_for(F&& f) {
  [&]<int... I>(std::integer_sequence<int, I...>) __attribute__((always_inline)) {
    (f(std::integral_constant<int, I>{}), ...);
  }(std::make_integer_sequence<int, N>{});
}

}  // namespace seunet
