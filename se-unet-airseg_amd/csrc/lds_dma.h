// LDS-DMA and counted waits of the marching kernels (conv_stream, conv_march, wgrad_stream, wgrad_march, wgrad_1x1): the one
// definition of the primitives and of the rules that every counted wait relies on.  Internal, device code only.
//
// One LDS-DMA wave-instruction copies 64 lanes x 16 B from global memory straight into the LDS at the M0 base + 16 * lane:
// no staging registers, no ds_write.  The instructions are inline asm, so the compiler neither counts nor drains them; a
// kernel waits for its own DMA with a counted `s_waitcnt vmcnt(N)` (wait_loads<N>) and for the other waves' parts with a raw
// s_barrier after it.  N is a compile-time count, and it is right only because of three facts:
//   (a) every wave issues the same number of DMA instructions per plane / step / chunk, whatever its share of the real data:
//       the surplus (padding) instructions read zero records (or the zero page) into a 1-KB dump slot of the LDS;
//   (b) a lane of the buffer form (dma16_buf) whose offset lies beyond num_records writes ZEROS into the LDS (probed on
//       gfx950: scripts/probes/blds_oob.hip).  So a padding voxel is a lane offset of 0xFFFFFFFF and a plane outside the
//       volume a descriptor of zero records: no zero page, no per-lane pointer select, no 64-bit address per instruction;
//   (c) a store may retire ahead of an older LDS-DMA load.  So N counts LOADS ONLY -- the DMA loads issued after the youngest
//       one being waited for -- and no store may be counted toward it, not even one issued between them (stores still in
//       flight only make the wait longer).  This departs from the MI355X microarchitecture guide (MI355X_MICROARCH.md), whose
//       wording is that loads, stores, atomics and LDS-DMA "count together, in issue order": a wait that also allowed the
//       stores issued since its plane let a step read a plane that had not landed, in about one launch of a hundred
//       ("the store path").
// Each kernel names its count (LOADS_PER_STEP or the like) and says next to each wait what is in flight there, and why.
#pragma once
#include <hip/hip_runtime.h>

namespace seunet {

typedef unsigned int rsrc_t __attribute__((ext_vector_type(4)));   // buffer descriptor: base lo, base hi (16 bits), num_records, word 3

// word 3 of every buffer descriptor here: data format 32 bit (bits 15..18 = 4), no swizzle, no stride index -- raw byte access
static constexpr unsigned RSRC_WORD3 = 0x00020000u;

__device__ __forceinline__ rsrc_t dma_rsrc(unsigned lo, unsigned hi, unsigned num_records) {
  rsrc_t r;
  r.x = lo; r.y = hi; r.z = num_records; r.w = RSRC_WORD3;
  return r;
}

// one LDS-DMA wave-instruction from a per-lane address: LDS destination = lds_dst + 16 * lane (M0 carries the base)
__device__ __forceinline__ void dma16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

// the same through a buffer descriptor: the 16 bytes of a lane come from base + soff + voff, see (b)
__device__ __forceinline__ void dma16_buf(unsigned voff, rsrc_t rsrc, unsigned soff, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(soff), "s"(lds_dst) : "memory");
}

// wait until at most N of this wave's vector-memory operations are outstanding; N counts DMA loads only, see (c)
template <int N> __device__ __forceinline__ void wait_loads() {
  static_assert(0 <= N && N <= 63, "vmcnt is a 6-bit counter");
  asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory");
}

}  // namespace seunet
