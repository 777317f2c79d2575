// Flat grid-stride passes (gfx950): layout conversion NCDHW <-> channels-last, the 2x2x2 max-pool and the zeroing of several
// small arrays in one launch.  All HBM-bound; one lane moves 8 channels (16/32 B).
//
//   max-pool      reference SE_UNet.py:131-133 (nn.MaxPool3d 2/2)
#include "seunet_common.h"
#include "wgrad.h"

namespace seunet {

// ---------------- layout ---------------------------------------------------------------------
template <typename T>
__global__ void pack_cl_kernel(const float* __restrict__ in, int C, T* __restrict__ out, int Cpad,
                               long long V, long long total) {
  // thread -> (n, group, v) with v fastest: coalesced f32 reads per channel plane
  const int G = Cpad / 8;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long v = i % V;
    const int g = (int)((i / V) % G);
    const long long n = i / (V * G);
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = g * 8 + j;
      x[j] = c < C ? in[(n * C + c) * V + v] : 0.f;
    }
    store8(out + (n * V + v) * Cpad + g * 8, x);
  }
}

template <typename T>
__global__ void unpack_cl_kernel(const T* __restrict__ in, int C, float* __restrict__ out, long long V,
                                 long long total) {
  const int G = C / 8;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long v = i % V;
    const int g = (int)((i / V) % G);
    const long long n = i / (V * G);
    float x[8];
    load8(in + (n * V + v) * C + g * 8, x);
#pragma unroll
    for (int j = 0; j < 8; ++j) out[(n * C + g * 8 + j) * V + v] = x[j];
  }
}

// ---------------- max-pool 2x2x2 ---------------------------------------------------------------
template <typename T>
__global__ void maxpool_fwd_kernel(const T* __restrict__ in, int C, T* __restrict__ out, int D, int H,
                                   int W, long long total) {
  const int G = C / 8, Do = D / 2, Ho = H / 2, Wo = W / 2;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int g = (int)(i % G);
    long long r = i / G;
    const int xo = (int)(r % Wo); r /= Wo;
    const int yo = (int)(r % Ho); r /= Ho;
    const int zo = (int)(r % Do);
    const long long n = r / Do;
    float m[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int z = 2 * zo + (k >> 2), y = 2 * yo + ((k >> 1) & 1), x = 2 * xo + (k & 1);
      float v[8];
      load8(in + ((((n * D + z) * H + y) * W + x) * (long long)C) + g * 8, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) m[j] = v[j] > m[j] ? v[j] : m[j];
    }
    store8(out + ((((n * Do + zo) * Ho + yo) * Wo + xo) * (long long)C) + g * 8, m);
  }
}

// routes g_out to the FIRST maximum of each window in (z,y,x) scan order (PyTorch CPU semantics)
template <typename T>
__global__ void maxpool_bwd_kernel(const T* __restrict__ in, const T* __restrict__ g_out, int C,
                                   T* g_in, int accumulate, int D, int H, int W, long long total) {
  const int G = C / 8, Do = D / 2, Ho = H / 2, Wo = W / 2;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int g = (int)(i % G);
    long long r = i / G;
    const int xo = (int)(r % Wo); r /= Wo;
    const int yo = (int)(r % Ho); r /= Ho;
    const int zo = (int)(r % Do);
    const long long n = r / Do;
    float m[8], gy[8];
    int am[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { m[j] = -INFINITY; am[j] = 0; }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int z = 2 * zo + (k >> 2), y = 2 * yo + ((k >> 1) & 1), x = 2 * xo + (k & 1);
      float v[8];
      load8(in + ((((n * D + z) * H + y) * W + x) * (long long)C) + g * 8, v);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (v[j] > m[j]) { m[j] = v[j]; am[j] = k; }
    }
    load8(g_out + ((((n * Do + zo) * Ho + yo) * Wo + xo) * (long long)C) + g * 8, gy);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int z = 2 * zo + (k >> 2), y = 2 * yo + ((k >> 1) & 1), x = 2 * xo + (k & 1);
      T* p = g_in + ((((n * D + z) * H + y) * W + x) * (long long)C) + g * 8;
      float v[8];
      if (accumulate) load8(p, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (accumulate ? v[j] : 0.f) + (am[j] == k ? gy[j] : 0.f);
      store8(p, v);
    }
  }
}

// ---------------- launchers -----------------------------------------------------------------------
int launch_pack_cl(int dtype, const float* in, int C, void* out, int Cpad, Dims d, hipStream_t s) {
  SEUNET_CHECK(Cpad % 8 == 0 && Cpad >= C, "pack_cl: padded channel count %d invalid for C=%d", Cpad, C);
  const long long V = d.vox(), total = (long long)d.N * V * (Cpad / 8);
  SEUNET_DTYPE_SWITCH(dtype, pack_cl_kernel<T><<<grid_for(total), 256, 0, s>>>(in, C, (T*)out, Cpad, V, total));
  SEUNET_LAUNCH_CHECK();
  return 0;
}
int launch_pack_input(int dtype, const float* x, int in_channel, void* out, Dims d, hipStream_t s) {
  SEUNET_CHECK(in_channel >= 1 && in_channel <= 8, "in_channel %d unsupported (1..8)", in_channel);
  return launch_pack_cl(dtype, x, in_channel, out, 8, d, s);
}
int launch_unpack_cl(int dtype, const void* in, int C, float* out, Dims d, hipStream_t s) {
  SEUNET_CHECK(C % 8 == 0, "unpack_cl: C=%d must be a multiple of 8", C);
  const long long V = d.vox(), total = (long long)d.N * V * (C / 8);
  SEUNET_DTYPE_SWITCH(dtype, unpack_cl_kernel<T><<<grid_for(total), 256, 0, s>>>((const T*)in, C, out, V, total));
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_maxpool_fwd(int dtype, const void* in, int C, void* out, Dims d, hipStream_t s) {
  SEUNET_CHECK(C % 8 == 0 && d.D % 2 == 0 && d.H % 2 == 0 && d.W % 2 == 0, "maxpool: bad shape");
  const long long total = (long long)d.N * (d.D / 2) * (d.H / 2) * (d.W / 2) * (C / 8);
  SEUNET_DTYPE_SWITCH(dtype, maxpool_fwd_kernel<T><<<grid_for(total), 256, 0, s>>>((const T*)in, C, (T*)out, d.D, d.H, d.W, total));
  SEUNET_LAUNCH_CHECK();
  return 0;
}
int launch_maxpool_bwd(int dtype, const void* in, const void* g_out, int C, void* g_in, int accumulate,
                       Dims d, hipStream_t s) {
  SEUNET_CHECK(C % 8 == 0 && d.D % 2 == 0 && d.H % 2 == 0 && d.W % 2 == 0, "maxpool: bad shape");
  const long long total = (long long)d.N * (d.D / 2) * (d.H / 2) * (d.W / 2) * (C / 8);
  SEUNET_DTYPE_SWITCH(dtype, maxpool_bwd_kernel<T><<<grid_for(total), 256, 0, s>>>((const T*)in, (const T*)g_out, C, (T*)g_in, accumulate, d.D, d.H, d.W, total));
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// zero several small f32 arrays with ONE launch (the identically-zero conv1.bias gradients of a backward pass: a
// hipMemsetAsync each is a 5-us fill kernel, thirty times per step).  The first launch can carry a rider (wgrad.h: the last
// weight gradient's slab reduction, at the end of the backward walk) as the blocks past its own; n = 0 with a rider is that
// reduction alone.
struct ZeroList { float* ptr[48]; int count[48]; int n; };
__global__ void __launch_bounds__(256) multi_zero_kernel(ZeroList z, WgReduceJob rider) {
  if ((int)blockIdx.x >= z.n) { wgrad_reduce_body(rider, (int)blockIdx.x - z.n); return; }
  float* p = z.ptr[blockIdx.x];
  for (int i = threadIdx.x; i < z.count[blockIdx.x]; i += blockDim.x) p[i] = 0.f;
}
int launch_multi_zero(float* const* ptrs, const int* counts, int n, hipStream_t s, const WgReduceJob* rider) {
  WgReduceJob job = rider ? *rider : WgReduceJob{};
  for (int base = 0; base < n || job.blocks() > 0; base += 48) {
    ZeroList z{};
    z.n = n - base < 48 ? n - base : 48;
    for (int i = 0; i < z.n; ++i) { z.ptr[i] = ptrs[base + i]; z.count[i] = counts[base + i]; }
    multi_zero_kernel<<<z.n + job.blocks(), 256, 0, s>>>(z, job);
    job = WgReduceJob{};
  }
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
