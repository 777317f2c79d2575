// Host-side layer of the forward / data-gradient convolution kernels (conv_igemm.hip: tiled and naive; conv_stream.hip;
// conv_march.hip): the family's interface.  A pass is routed to a kernel once (ConvKernel; net.cpp, Plan::route) and
// everything about it that depends on the kernel -- whether it serves the shape, the bytes of its packed weight, its
// statistics slots, packing the weight, the launch -- is asked here with that kernel as the first argument (conv.cpp).
// A kernel file contributes its launch cut, its own predicate and sizes, one list-packing launcher and its launcher.
#pragma once
#include "seunet_common.h"

namespace seunet {

// the kernel of each conv pass, the weight gradients' included (wgrad.h); the values are SEUNET_KERNEL_* (net.cpp)
enum class ConvKernel { Naive, Tiled, Stream, March, Wgrad1x1 };

// ---- the family, by kernel (conv.cpp) ----
// Stream: one source and one destination that conv_stream_supported takes; March: conv_march_supported; Tiled / Naive: true
bool conv_supported(ConvKernel k, int dtype, int taps, int dil, const SrcList& src, const DstList& dst);
// bytes of a packed weight: src_c channels in the single source tensor (Stream), cin -> cout channels
size_t conv_wpack_bytes(ConvKernel k, int dtype, int taps, int src_c, int cin, int cout);
// statistics slots per sample of a forward conv
int conv_slots(ConvKernel k, Dims d, int taps, int dil, int cin, int cout);
// one forward or data-gradient conv.  w_torch: the PyTorch weight (naive kernel, tflip 1 = data gradient); wpack: the weight
// packed for k by launch_conv_pack
int run_conv(ConvKernel k, int dtype, int taps, int dil, const SrcList& src, int cin_logical, const float* w_torch, int tflip,
             const void* wpack, const float* bias, const DstList& dst, double* stats, Dims d, hipStream_t s);
// PyTorch weight w (cout_w, cin_w, k, k, k) -> wpack in k's MFMA layout, read transposed / mirrored by the data gradient
// (tflip); src_c -> dst_c: the channels of the conv's source and destination tensors (Stream, March)
struct ConvPackJob { ConvKernel k; const float* w; void* wpack; int taps, cin_w, cout_w, tflip, src_c, dst_c; };
// every weight of a pass in one launch per kernel and list: the Stream jobs, then March, then Tiled; Naive jobs pack nothing
int launch_conv_pack(int dtype, const ConvPackJob* jobs, int n, hipStream_t s);

// a kernel's jobs `cap` at a time (the entries of its list struct, a kernel-argument size): launch(first job, count) fills one
// list and launches it, and every launch is checked
template <class F> static int conv_pack_chunks(const ConvPackJob* jobs, int n, int cap, F launch) {
  for (int i0 = 0; i0 < n; i0 += cap) {
    if (int e = launch(jobs + i0, n - i0 < cap ? n - i0 : cap)) return e;
    SEUNET_LAUNCH_CHECK();
  }
  return 0;
}

// ---- tiled and naive kernels (conv_igemm.hip) ----
size_t conv_igemm_wpack_bytes(int dtype, int taps, int cin, int cout);
int conv_stats_tiles(Dims d, int taps, int dil);   // partial-stat slots per sample written by the igemm kernel
int launch_conv_igemm_pack(int dtype, const ConvPackJob* jobs, int n, hipStream_t s);
int launch_conv_igemm(int dtype, int taps, int dil, const SrcList& src, int cin_logical,
                      const void* wpack, const float* bias, const DstList& dst,
                      double* stats_partial, Dims d, hipStream_t s);
int launch_conv_naive(int dtype, int taps, int dil, const SrcList& src, int cin_logical,
                      const float* w_torch, int transpose_flip, const float* bias,
                      const DstList& dst, Dims d, hipStream_t s);

// ---- streaming small-channel 3x3x3 convolution (conv_stream.hip): bf16 | f16, 8/16/32 source channels, <= 32 destination
// channels ----
bool conv_stream_supported(int dtype, int taps, int dil, int src_c, int dst_c);
size_t conv_stream_wpack_bytes(int src_c);
int conv_stream_slots(Dims d, int dil);
int launch_conv_stream_pack(int dtype, const ConvPackJob* jobs, int n, hipStream_t s);
int launch_conv_stream(int dtype, int dil, const void* src, int src_c, const void* wpack, const float* bias, void* dst, int dst_c,
                       int dst_accumulate, double* stats, Dims d, hipStream_t s);

// ---- marching 3x3x3 convolution for 32 / 64 source channels (conv_march.hip): bf16 | f16, one or two equal sources,
// destinations in multiples of 16 channels; forward (bias, statistics) and data gradient (optionally accumulating) ----
bool conv_march_supported(int dtype, int taps, int dil, const SrcList& src, const DstList& dst);
size_t conv_march_wpack_bytes(int cin_e, int cout_e);
int conv_march_slots(Dims d, int dil, int cin_e, int cout_e);
int launch_conv_march_pack(int dtype, const ConvPackJob* jobs, int n, hipStream_t s);
int launch_conv_march(int dtype, int dil, const SrcList& src, const void* wpack, const float* bias, const DstList& dst, double* stats,
                      Dims d, hipStream_t s);

}  // namespace seunet
