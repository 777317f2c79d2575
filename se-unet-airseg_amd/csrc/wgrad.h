// Host-side layer of the weight-gradient kernels (wgrad.hip: tiled and naive; wgrad_march.hip; wgrad_1x1.hip; wgrad_stream.hip):
// the family's interface, and the two things all four matrix-core kernels do alike.  Each keeps ONE slab of f32 accumulators
// per persistent workgroup in the caller's workspace (the slab convention, WgSlabs), and a second launch adds the slabs in f64
// in a fixed order into the PyTorch layout (wgrad_reduce_body: deterministic, no atomics).  A kernel file contributes its
// launch cut and nothing else of this; its Map -- where element e of a slab lies in dW -- is here too, since the reduction
// travels as one struct (WgReduceJob).
#pragma once
#include "conv.h"

namespace seunet {

struct WgReduceJob;   // the reduction of a launch's slabs, as data (below)

// ---- the family (ConvKernel: conv.h) ----
// streaming small-channel weight gradient (wgrad_stream.hip)
bool wgrad_stream_supported(int dtype, int taps, int dil, int x_c, int dy_c);
size_t wgrad_stream_workspace_bytes(int x_c, int dy_c, int dil, Dims d);
int launch_wgrad_stream(int dtype, int dil, const void* x, int x_c, int cin_w, const void* dy, int dy_c, int cout_w, float* dw,
                        void* workspace, size_t ws_bytes, Dims d, hipStream_t s, WgReduceJob* defer = nullptr);

// weight gradient (wgrad.hip).  The workspace serves whichever weight-gradient kernel the layer is routed to: the most any of
// them needs for these channels (the tiled kernel's slabs, wgrad_1x1_workspace_bytes, wgrad_march_workspace_bytes)
static constexpr int WG_TILED_SLABS = 512;   // slabs of the tiled kernel over all (ci, co) combos: two workgroups per CU
size_t wgrad_workspace_bytes(int taps, int cin, int cout);
int launch_wgrad(int dtype, int taps, int dil, const SrcList& x, int cin_logical, const void* dy,
                 int cout, float* dw_torch, void* workspace, size_t ws_bytes, Dims d, hipStream_t s, WgReduceJob* defer = nullptr);
// marching weight gradient (wgrad_march.hip); src_dist: byte distance between the two sources of x (32-bit reach)
bool wgrad_march_supported(int dtype, int taps, int dil, const SrcList& x, int cin_logical, int cout, Dims d, long long src_dist);
int launch_wgrad_march(int dtype, int taps, int dil, const SrcList& x, int cin_logical, const void* dy, int cout,
                       float* dw, void* workspace, size_t ws_bytes, Dims d, hipStream_t s, WgReduceJob* defer = nullptr);
size_t wgrad_march_workspace_bytes(int taps, int cin, int cout);   // its bound for any volume; 0 for channels it does not take
// 1x1x1 weight gradient of the aggregation convolutions (wgrad_1x1.hip)
bool wgrad_1x1_supported(int dtype, const SrcList& x, int cin_logical, int cout);
int launch_wgrad_1x1(int dtype, const SrcList& x, int cin_logical, const void* dy, int cout, float* dw, void* workspace,
                     size_t ws_bytes, Dims d, hipStream_t s, WgReduceJob* defer = nullptr);
size_t wgrad_1x1_workspace_bytes(int cin, int cout);               // its bound for any volume
int launch_wgrad_naive(int dtype, int taps, int dil, const SrcList& x, int cin_logical,
                       const void* dy, int cout, float* dw_torch, Dims d, hipStream_t s);
// the non-streaming weight gradient's choice by size (net.cpp, kernel routing: the network plan and seunet_conv3d_wgrad);
// src_dist as above
ConvKernel wgrad_kernel(int dtype, int taps, int dil, const SrcList& x, int cin_logical, int cout, Dims d, long long src_dist);
// weight gradient on kernel k (Stream: one source, dy with cout channels); wgrad.hip, next to wgrad_workspace_bytes.
// defer null: dw is written when the call's launches have run.  Non-null: the slabs are written, the reduction into dw is
// handed back as a job that the caller must run (launch_wgrad_reduce, or as a rider of another launch) before anything
// reads dw or writes the workspace; the naive kernel has no reduction and leaves *defer alone.
int run_wgrad(ConvKernel k, int dtype, int taps, int dil, const SrcList& x, int cin_logical, const void* dy, int cout, float* dw,
              void* workspace, size_t ws_bytes, Dims d, hipStream_t s, WgReduceJob* defer = nullptr);

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
// ---- where element e of a slab lies in dW: one Map per kernel ----
// map(combo, e): the index into dw of element e of a slab of that combo, negative for an element of the channel padding.
// tiled kernel (wgrad.hip): e = (tap, ci, co) of a slab of the 32 x 32 combo -> dW (cout_w, cin_w, taps)
struct WgMap {
  int taps, cin_w, cout_w, co_tiles;
  __device__ long long operator()(int combo, int e) const {
    const int tap = e >> 10, ci = (combo / co_tiles) * 32 + ((e >> 5) & 31), co = (combo % co_tiles) * 32 + (e & 31);
    return ci < cin_w && co < cout_w ? (long long)(((size_t)co * cin_w + ci) * taps + tap) : -1;
  }
};
// marching kernel (wgrad_march.hip): e = (pair, tap, lane, component) of a slab of the (xc x yc)-channel combo
// -> dW (cout, cin_w, 27); no channel padding
struct WmMap {
  int ncb, pw, xc, yc, nco, cin_w;
  __device__ long long operator()(int combo, int e) const {
    const int comp = e & 3, lane = (e >> 2) & 63, tap = (e >> 8) % 27, pair = e / (27 * 256);
    const int wave = pair / pw, kk = pair % pw;
    const int cib = wave % ncb, cob = (wave / ncb) * pw + kk;
    const int co = (combo % nco) * yc + cob * 16 + 4 * (lane >> 4) + comp;
    const int ci = (combo / nco) * xc + cib * 16 + (lane & 15);
    return (long long)(((size_t)co * cin_w + ci) * 27 + tap);
  }
};
// streaming kernel (wgrad_stream.hip): e = (tap, ci, co) of a slab [27][cin][cout] (one combo) -> dW (cout_w, cin_w, 3, 3, 3)
struct WsMap {
  int cin, cout, cin_w, cout_w;
  __device__ long long operator()(int, int e) const {
    const int co = e % cout, ci = (e / cout) % cin, tap = e / (cout * cin);
    return ci < cin_w && co < cout_w ? (long long)(((size_t)co * cin_w + ci) * 27 + tap) : -1;
  }
};
// 1x1x1 kernel (wgrad_1x1.hip): e = (wave, input block, output block, lane, component) of a slab (one combo: all channels)
// -> dW (cout, cin)
struct W1Map {
  int cibw, ncob, cin;
  __device__ long long operator()(int, int e) const {
    const int comp = e & 3, lane = (e >> 2) & 63, pair = e >> 8;
    const int kk = pair % ncob, c = (pair / ncob) % cibw, wave = pair / (ncob * cibw);
    const int co = kk * 16 + 4 * (lane >> 4) + comp;
    const int ci = (wave * cibw + c) * 16 + (lane & 15);
    return ci < cin ? (long long)((size_t)co * cin + ci) : -1;
  }
};

// ---- the reduction ----
// dW (PyTorch layout) = fixed-order sum of the `nslab` slabs of each combo.  The reduction is data (WgReduceJob), so that it
// need not be a launch of its own: a launcher either runs it at once (wgrad_reduce_kernel) or hands the job back (`defer`),
// and the network's backward walk lets it ride the next block's finalize launch as extra workgroups (net.cpp, `pending`).
// Nothing reads a weight gradient before the end of the backward, and the slabs stay put until the next weight gradient.
struct WgReduceJob {
  enum Kind { None, Tiled, March, Stream, One } kind = None;
  const float* slab = nullptr;
  int nslab = 0, per = 0, combos = 0;
  float* dw = nullptr;
  union { WgMap g; WmMap m; WsMap s; W1Map o; } map = {};
  void set(const WgMap& v) { kind = Tiled; map.g = v; }
  void set(const WmMap& v) { kind = March; map.m = v; }
  void set(const WsMap& v) { kind = Stream; map.s = v; }
  void set(const W1Map& v) { kind = One; map.o = v; }
  __host__ __device__ int blocks_per_combo() const { return (per + 63) / 64; }
  int blocks() const { return kind == None ? 0 : combos * blocks_per_combo(); }   // 256-thread workgroups of the job
};

// A 256-thread block owns 64 consecutive slab elements (the bx-th sixty-four of combo `combo`), each thread four of them (one
// 16-byte load per slab; `per` is a multiple of 4 and the slabs are 16-byte aligned, finish_wgrad).  Its 16 thread groups each
// sum every 16th slab (256-B coalesced reads, 16-fold shorter dependent chains than one thread per element: that version
// averaged 37 us per launch, ~1 ms per training step), on two chains per element, and the 16 partial sums of an element are
// combined in group order through LDS.  The order of summation of an element is that of the 16-element blocks this replaced:
// the same bits.  f64 throughout; deterministic, no atomics.
static constexpr int WG_RED_PAD = 65;
template <typename Map>
__device__ __forceinline__ void wgrad_reduce_elements(const float* __restrict__ slab, int nslab, int per, const Map& map,
                                                      float* __restrict__ dw, int bx, int combo, double (&red)[16][WG_RED_PAD]) {
  const int quad = threadIdx.x & 15, part = threadIdx.x >> 4;
  const int e0 = bx * 64 + quad * 4;      // first of this thread's four elements inside one slab
  double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
  if (e0 < per) {
    const float* p = slab + (size_t)combo * nslab * per + e0;
    int k = part;
    for (; k + 16 < nslab; k += 32) {
      const float4 a = *reinterpret_cast<const float4*>(p + (size_t)k * per);
      const float4 b = *reinterpret_cast<const float4*>(p + (size_t)(k + 16) * per);
      s0[0] += (double)a.x; s0[1] += (double)a.y; s0[2] += (double)a.z; s0[3] += (double)a.w;
      s1[0] += (double)b.x; s1[1] += (double)b.y; s1[2] += (double)b.z; s1[3] += (double)b.w;
    }
    if (k < nslab) {
      const float4 a = *reinterpret_cast<const float4*>(p + (size_t)k * per);
      s0[0] += (double)a.x; s0[1] += (double)a.y; s0[2] += (double)a.z; s0[3] += (double)a.w;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[part][quad * 4 + j] = s0[j] + s1[j];
  __syncthreads();
  const int el = threadIdx.x, e = bx * 64 + el;
  if (el < 64 && e < per) {
    const long long i = map(combo, e);
    if (i >= 0) {
      double t = red[0][el];
#pragma unroll
      for (int q = 1; q < 16; ++q) t += red[q][el];
      dw[i] = (float)t;
    }
  }
}

// workgroup `block` of job.blocks(): combo = block / cdiv(per, 64).  Uniform per workgroup; a host kernel calls it for the
// workgroups past its own (gate_bwd_finalize_kernel, cat_bwd_finalize_kernel, multi_zero_kernel) and returns.
__device__ __forceinline__ void wgrad_reduce_body(const WgReduceJob& job, int block) {
  __shared__ double red[16][WG_RED_PAD];
  const int bpc = job.blocks_per_combo();
  const int combo = block / bpc, bx = block % bpc;
  switch (job.kind) {
    case WgReduceJob::Tiled: wgrad_reduce_elements(job.slab, job.nslab, job.per, job.map.g, job.dw, bx, combo, red); break;
    case WgReduceJob::March: wgrad_reduce_elements(job.slab, job.nslab, job.per, job.map.m, job.dw, bx, combo, red); break;
    case WgReduceJob::Stream: wgrad_reduce_elements(job.slab, job.nslab, job.per, job.map.s, job.dw, bx, combo, red); break;
    case WgReduceJob::One: wgrad_reduce_elements(job.slab, job.nslab, job.per, job.map.o, job.dw, bx, combo, red); break;
    default: break;
  }
}

// the job a launcher has just filled: handed back through `defer`, or run now as a launch of its own (wgrad.hip)
int launch_wgrad_reduce(const WgReduceJob& job, hipStream_t s);
template <typename Map>
static int finish_wgrad(const float* slab, int nslab, int per, int combos, const Map& map, float* dw, WgReduceJob* defer,
                        hipStream_t s) {
  SEUNET_CHECK(per % 4 == 0 && (reinterpret_cast<uintptr_t>(slab) & 15) == 0,
               "wgrad: the slab reduction reads 16 bytes at a time (slab of %d floats at %p)", per, (const void*)slab);
  WgReduceJob job;
  job.slab = slab; job.nslab = nslab; job.per = per; job.combos = combos; job.dw = dw;
  job.set(map);
  if (defer) { *defer = job; return 0; }
  return launch_wgrad_reduce(job, s);
}
#endif  // __HIPCC__

}  // namespace seunet
