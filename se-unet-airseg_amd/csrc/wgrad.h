// Host-side layer of the weight-gradient kernels (wgrad.hip: tiled and naive; wgrad_march.hip; wgrad_1x1.hip; wgrad_stream.hip):
// the family's interface, and the two things all four matrix-core kernels do alike.  Each keeps ONE slab of f32 accumulators
// per persistent workgroup in the caller's workspace (the slab convention, WgSlabs), and a second launch adds the slabs in f64
// in a fixed order into the PyTorch layout (wgrad_reduce_kernel: deterministic, no atomics).  A kernel file contributes its
// launch cut and its Map -- where element e of a slab lies in dW -- and nothing else of this.
#pragma once
#include "seunet_common.h"

namespace seunet {

// ---- the family (ConvKernel, the enum the routing speaks in, is in seunet_common.h: the forward convs use it too) ----
// streaming small-channel weight gradient (wgrad_stream.hip)
bool wgrad_stream_supported(int dtype, int taps, int dil, int x_c, int dy_c);
size_t wgrad_stream_workspace_bytes(int x_c, int dy_c, int dil, Dims d);
int launch_wgrad_stream(int dtype, int dil, const void* x, int x_c, int cin_w, const void* dy, int dy_c, int cout_w, float* dw,
                        void* workspace, size_t ws_bytes, Dims d, hipStream_t s);

// weight gradient (wgrad.hip).  The workspace serves whichever weight-gradient kernel the layer is routed to: the most any of
// them needs for these channels (the tiled kernel's slabs, wgrad_1x1_workspace_bytes, wgrad_march_workspace_bytes)
static constexpr int WG_TILED_SLABS = 512;   // slabs of the tiled kernel over all (ci, co) combos: two workgroups per CU
size_t wgrad_workspace_bytes(int taps, int cin, int cout);
int launch_wgrad(int dtype, int taps, int dil, const SrcList& x, int cin_logical, const void* dy,
                 int cout, float* dw_torch, void* workspace, size_t ws_bytes, Dims d, hipStream_t s);
// marching weight gradient (wgrad_march.hip); src_dist: byte distance between the two sources of x (32-bit reach)
bool wgrad_march_supported(int dtype, int taps, int dil, const SrcList& x, int cin_logical, int cout, Dims d, long long src_dist);
int launch_wgrad_march(int dtype, int taps, int dil, const SrcList& x, int cin_logical, const void* dy, int cout,
                       float* dw, void* workspace, size_t ws_bytes, Dims d, hipStream_t s);
size_t wgrad_march_workspace_bytes(int taps, int cin, int cout);   // its bound for any volume; 0 for channels it does not take
// 1x1x1 weight gradient of the aggregation convolutions (wgrad_1x1.hip)
bool wgrad_1x1_supported(int dtype, const SrcList& x, int cin_logical, int cout);
int launch_wgrad_1x1(int dtype, const SrcList& x, int cin_logical, const void* dy, int cout, float* dw, void* workspace,
                     size_t ws_bytes, Dims d, hipStream_t s);
size_t wgrad_1x1_workspace_bytes(int cin, int cout);               // its bound for any volume
int launch_wgrad_naive(int dtype, int taps, int dil, const SrcList& x, int cin_logical,
                       const void* dy, int cout, float* dw_torch, Dims d, hipStream_t s);
// the non-streaming weight gradient's choice by size (net.cpp, kernel routing: the network plan and seunet_conv3d_wgrad);
// src_dist as above
ConvKernel wgrad_kernel(int dtype, int taps, int dil, const SrcList& x, int cin_logical, int cout, Dims d, long long src_dist);
// weight gradient on kernel k (Stream: one source, dy with cout channels); wgrad.hip, next to wgrad_workspace_bytes
int run_wgrad(ConvKernel k, int dtype, int taps, int dil, const SrcList& x, int cin_logical, const void* dy, int cout, float* dw,
              void* workspace, size_t ws_bytes, Dims d, hipStream_t s);

// ---- the slab convention ----
// A launch keeps `nslab` slabs (over all its channel combos; slab (combo * slabs-per-combo + workgroup)) of `per` floats each,
// back to back, `prefix` bytes into the workspace.  Every workspace query is bytes(), every launcher takes its slab pointer
// from base(), which is also its size check.
//
// WG_SLAB_PREFIX: the tiled, marching and 1x1x1 kernels skip the first 256 bytes of the workspace.  They used to be the zero
// page that padding reads; that page is device_zero_page() now and nothing reads or writes these bytes.  They stay because the
// workspace sizes are pinned (tests/test_launch_cut_host.py: WGRAD_BYTES and the arena sizes).  The streaming kernel never
// had them: its prefix is 0.
static constexpr size_t WG_SLAB_PREFIX = 256;
struct WgSlabs {
  size_t prefix, nslab, per;
  size_t bytes() const { return prefix + nslab * per * sizeof(float); }
  float* base(void* workspace, size_t ws_bytes) const {   // nullptr: the workspace is too small
    return ws_bytes >= bytes() ? reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(workspace) + prefix) : nullptr;
  }
};

#ifdef __HIPCC__
// ---- the reduction ----
// dW (PyTorch layout) = fixed-order sum of the `nslab` slabs of each combo (blockIdx.y).  A 256-thread block owns 16 consecutive
// slab elements; its 16 thread groups each sum every 16th slab (64-B coalesced reads, 16-fold shorter dependent chains than
// one thread per element: that version averaged 37 us per launch, ~1 ms per training step), on two chains, and the 16 partial
// sums are combined in group order through LDS.  f64 throughout; deterministic, no atomics.
// map(combo, e): the index into dw of element e of a slab of that combo, negative for an element of the channel padding.
template <typename Map>
__global__ void __launch_bounds__(256)
wgrad_reduce_kernel(const float* __restrict__ slab, int nslab, int per, Map map, float* __restrict__ dw) {
  const int el = threadIdx.x & 15, part = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + el;             // element inside one slab
  const int combo = blockIdx.y;
  double s0 = 0.0, s1 = 0.0;
  if (e < per) {
    const float* p = slab + (size_t)combo * nslab * per + e;
    int k = part;
    for (; k + 16 < nslab; k += 32) {
      s0 += (double)p[(size_t)k * per];
      s1 += (double)p[(size_t)(k + 16) * per];
    }
    if (k < nslab) s0 += (double)p[(size_t)k * per];
  }
  __shared__ double red[16][17];
  red[part][el] = s0 + s1;
  __syncthreads();
  if (part == 0 && e < per) {
    const long long i = map(combo, e);
    if (i >= 0) {
      double t = red[0][el];
#pragma unroll
      for (int q = 1; q < 16; ++q) t += red[q][el];
      dw[i] = (float)t;
    }
  }
}

template <typename Map>
static int launch_wgrad_reduce(const float* slab, int nslab, int per, int combos, Map map, float* dw, hipStream_t s) {
  wgrad_reduce_kernel<Map><<<dim3(cdiv(per, 16), combos), 256, 0, s>>>(slab, nslab, per, map, dw);
  SEUNET_LAUNCH_CHECK();
  return 0;
}
#endif  // __HIPCC__

}  // namespace seunet
