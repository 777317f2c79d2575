// Gradient of the loss with respect to the network input x (N, in_channel, D, H, W) -- seunet_net_backward_input, net.cpp.
// x feeds four places (reference SE_UNet.py:183-205): ec1's 3x3x3 conv, x33 (1x1x1 at full resolution), x63 on pool0(x) and
// x93 on pool1(pool0(x)), so
//
//   dL/dx = convT_ec1(draw_ec1) + W_x33^T d2_x33 + unpool_0( W_x63^T d2_x63 + unpool_1( W_x93^T d2_x93 ) )
//
// The per-level x-branch terms gx_l = W_xl^T d2_xl ([N][V_l][in_channel] f32) come from pass B of the aggregation block
// (cat.hip cat_bwd_kernel XG when the branch is recomputed from the input; xgrad_contract_kernel below from the stored
// d2 otherwise).  unpool_l routes to the FIRST strict maximum of each 2x2x2 window of the stored input copy (feat[T_X0] /
// feat[T_X1]), the forward's own rule (layout.hip maxpool_bwd_kernel).  In bf16 / fp16 storage the network computes on its
// rounded copy of x: this is the gradient with respect to that copy, the rounding passed straight through.
// Everything here is f32, written once per element (no atomics): the result is deterministic.
#include "seunet_common.h"

namespace seunet {

// gx[n][v][k] (+)= sum_c d2[n][v][c] * W2[c][k]   (d2 channel-last in the storage type, W2 PyTorch (C, in_channel, 1, 1, 1))
template <typename T>
__global__ void __launch_bounds__(256)
xgrad_contract_kernel(const T* __restrict__ d2, int C, const float* __restrict__ w2, int ic, float* __restrict__ gx, int accumulate,
                      long long total) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    float p[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = 0.f;
    for (int c = 0; c < C; c += 8) {
      float v[8];
      load8(d2 + i * C + c, v);
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k < ic) p[k] = fmaf(v[j], w2[(c + j) * ic + k], p[k]);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < ic) gx[i * ic + k] = accumulate ? gx[i * ic + k] + p[k] : p[k];
  }
}

// gx_fine[n][v][k] = (v is the first maximum of its window in channel k of x_fine) ? gx_coarse[n][window][k] : 0   (one thread per
// window writes all eight of its voxels: every fine element is written exactly once)
template <typename T>
__global__ void __launch_bounds__(256)
xgrad_unpool_kernel(const T* __restrict__ xf, int ic, const float* __restrict__ gxc, float* __restrict__ gxf, int D, int H, int W,
                    long long total) {
  const int Do = D / 2, Ho = H / 2, Wo = W / 2;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long r = i;
    const int xo = (int)(r % Wo); r /= Wo;
    const int yo = (int)(r % Ho); r /= Ho;
    const int zo = (int)(r % Do);
    const long long n = r / Do;
    float m[8];
    int am[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { m[j] = -INFINITY; am[j] = 0; }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int z = 2 * zo + (q >> 2), y = 2 * yo + ((q >> 1) & 1), x = 2 * xo + (q & 1);
      float v[8];
      load8(xf + (((n * D + z) * H + y) * W + x) * 8, v);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (v[j] > m[j]) { m[j] = v[j]; am[j] = q; }
    }
    float g[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] = k < ic ? gxc[i * ic + k] : 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int z = 2 * zo + (q >> 2), y = 2 * yo + ((q >> 1) & 1), x = 2 * xo + (q & 1);
      float* o = gxf + (((n * D + z) * H + y) * W + x) * ic;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < ic) o[k] = am[k] == q ? g[k] : 0.f;
    }
  }
}

// Full resolution, one thread per output voxel, a 4 x 8 x 8 tile per workgroup:
//   grad_x[n][k][v] = sum_{tap, c} draw[v - tap + 1][c] * W_ec1[c][k][tap]   (the 3x3x3 transposed conv, dilation 1, zero outside)
//                   + gx0[n][v][k]
//                   + (v is the first maximum of its window in channel k of x0 ? gx1[n][window(v)][k] : 0)
// draw (ec1's raw-output gradient, channel-last, CE = 8 * width_mult channels) is staged through LDS as f32 with a one-voxel halo
// (6 x 10 x 10 voxels); the weights are uniform across the workgroup (scalar loads).  VALU f32 FMAs: with N = in_channel <= 2 an
// MFMA tile would be mostly padding.
constexpr int IG_TZ = 4, IG_TY = 8, IG_TX = 8, IG_HZ = IG_TZ + 2, IG_HY = IG_TY + 2, IG_HX = IG_TX + 2;
constexpr int IG_HALO = IG_HZ * IG_HY * IG_HX;
template <typename T, int IC, int CE>
__global__ void __launch_bounds__(256)
input_grad_kernel(const T* __restrict__ draw, const float* __restrict__ w, const T* __restrict__ x0, const float* __restrict__ gx0,
                  const float* __restrict__ gx1, float* __restrict__ grad_x, int D, int H, int W) {
  __shared__ __attribute__((aligned(16))) float s_src[IG_HALO * CE];
  const int tilesx = W / IG_TX;
  const int x0t = (blockIdx.x % tilesx) * IG_TX, y0t = (blockIdx.x / tilesx) * IG_TY, z0t = blockIdx.y * IG_TZ;
  const long long n = blockIdx.z;
  const long long V = (long long)D * H * W;
  constexpr int G = CE / 8;
  for (int i = threadIdx.x; i < IG_HALO * G; i += 256) {
    const int hv = i / G, g = i % G;
    const int hz = hv / (IG_HY * IG_HX), hy = (hv / IG_HX) % IG_HY, hx = hv % IG_HX;
    const int z = z0t + hz - 1, y = y0t + hy - 1, x = x0t + hx - 1;
    float v[8];
    if (z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W) {
      load8(draw + (n * V + ((long long)z * H + y) * W + x) * CE + g * 8, v);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
    }
    float4* d = reinterpret_cast<float4*>(s_src + hv * CE + g * 8);
    d[0] = make_float4(v[0], v[1], v[2], v[3]);
    d[1] = make_float4(v[4], v[5], v[6], v[7]);
  }
  __syncthreads();
  const int tx = threadIdx.x % IG_TX, ty = (threadIdx.x / IG_TX) % IG_TY, tz = threadIdx.x / (IG_TX * IG_TY);
  float acc[IC];
#pragma unroll
  for (int k = 0; k < IC; ++k) acc[k] = 0.f;
  // (one (a, b) row of three taps per iteration: its 3 * CE * IC weights come in by scalar loads; unrolling all 27 taps put every
  // weight in SGPRs at once and spilled them)
#pragma unroll 1
  for (int a = 0; a < 3; ++a)
#pragma unroll 1
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int tap = (a * 3 + b) * 3 + c;
        const float* sp = s_src + (((tz + 2 - a) * IG_HY + (ty + 2 - b)) * IG_HX + (tx + 2 - c)) * CE;
#pragma unroll
        for (int q = 0; q < CE; q += 4) {
          const float4 s4 = *reinterpret_cast<const float4*>(sp + q);
          const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < IC; ++k) acc[k] = fmaf(sv[j], w[((q + j) * IC + k) * 27 + tap], acc[k]);
        }
      }
  const int z = z0t + tz, y = y0t + ty, x = x0t + tx;
  const long long v = ((long long)z * H + y) * W + x;
  // the two x-branch terms: this level's, and the half-resolution one where this voxel was its window's first maximum
  const int kpos = ((z & 1) << 2) | ((y & 1) << 1) | (x & 1);
  float m[8];
  int am[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { m[j] = -INFINITY; am[j] = 0; }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int zz = (z & ~1) + (q >> 2), yy = (y & ~1) + ((q >> 1) & 1), xx = (x & ~1) + (q & 1);
    float xv[8];
    load8(x0 + (n * V + ((long long)zz * H + yy) * W + xx) * 8, xv);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (xv[j] > m[j]) { m[j] = xv[j]; am[j] = q; }
  }
  const long long V1 = V / 8;
  const long long parent = ((long long)(z >> 1) * (H >> 1) + (y >> 1)) * (W >> 1) + (x >> 1);
#pragma unroll
  for (int k = 0; k < IC; ++k) {
    float g = acc[k] + gx0[(n * V + v) * IC + k];
    if (am[k] == kpos) g += gx1[(n * V1 + parent) * IC + k];
    grad_x[(n * IC + k) * V + v] = g;
  }
}

static inline int ig_grid(long long total) {
  long long b = (total + 255) / 256;
  return (int)(b < 65536 ? (b < 1 ? 1 : b) : 65536);
}

int launch_xgrad_contract(int dtype, const void* d2, int C, const float* w2, int in_channel, float* gx, int accumulate, Dims d,
                          hipStream_t s) {
  SEUNET_CHECK(d2 && w2 && gx && C % 8 == 0 && C > 0 && in_channel >= 1 && in_channel <= 8, "xgrad_contract: bad argument");
  const long long total = (long long)d.N * d.vox();
  SEUNET_DTYPE_SWITCH(dtype, xgrad_contract_kernel<T><<<ig_grid(total), 256, 0, s>>>((const T*)d2, C, w2, in_channel, gx, accumulate, total));
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_xgrad_unpool(int dtype, const void* x_fine, int in_channel, const float* gx_coarse, float* gx_fine, Dims fine, hipStream_t s) {
  SEUNET_CHECK(x_fine && gx_coarse && gx_fine && in_channel >= 1 && in_channel <= 8, "xgrad_unpool: bad argument");
  SEUNET_CHECK(fine.D % 2 == 0 && fine.H % 2 == 0 && fine.W % 2 == 0, "xgrad_unpool: extents (%d,%d,%d) must be even", fine.D, fine.H, fine.W);
  const long long total = (long long)fine.N * fine.vox() / 8;
  SEUNET_DTYPE_SWITCH(dtype, xgrad_unpool_kernel<T><<<ig_grid(total), 256, 0, s>>>((const T*)x_fine, in_channel, gx_coarse, gx_fine, fine.D,
                                                                                  fine.H, fine.W, total));
  SEUNET_LAUNCH_CHECK();
  return 0;
}

template <typename T, int CE>
static int input_grad_ic(const void* draw, const float* w, const void* x0, int ic, const float* gx0, const float* gx1, float* grad_x,
                         Dims d, dim3 grid, hipStream_t s) {
#define SEUNET_IG_CASE(K)                                                                                                         \
  case K:                                                                                                                         \
    input_grad_kernel<T, K, CE><<<grid, 256, 0, s>>>((const T*)draw, w, (const T*)x0, gx0, gx1, grad_x, d.D, d.H, d.W);          \
    break;
  switch (ic) {
    SEUNET_IG_CASE(1) SEUNET_IG_CASE(2) SEUNET_IG_CASE(3) SEUNET_IG_CASE(4)
    SEUNET_IG_CASE(5) SEUNET_IG_CASE(6) SEUNET_IG_CASE(7) SEUNET_IG_CASE(8)
    default: return fail("input_grad: in_channel %d (1 .. 8)", ic);
  }
#undef SEUNET_IG_CASE
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_input_grad(int dtype, const void* draw, int ce, const float* w_ec1, const void* x0, int in_channel, const float* gx0,
                      const float* gx1, float* grad_x, Dims d, hipStream_t s) {
  SEUNET_CHECK(draw && w_ec1 && x0 && gx0 && gx1 && grad_x, "input_grad: null argument");
  SEUNET_CHECK(ce == 8 || ce == 16, "input_grad: ec1 has %d output channels (8 or 16)", ce);
  SEUNET_CHECK(d.D % IG_TZ == 0 && d.H % IG_TY == 0 && d.W % IG_TX == 0,
               "input_grad: extents (%d,%d,%d) must be multiples of (%d,%d,%d)", d.D, d.H, d.W, IG_TZ, IG_TY, IG_TX);
  const long long tiles_xy = (long long)(d.W / IG_TX) * (d.H / IG_TY);
  SEUNET_CHECK(tiles_xy < (1ll << 31) && d.D / IG_TZ <= 65535 && d.N <= 65535,
               "input_grad: grid (%lld, %d, %d) exceeds the launch limits", tiles_xy, d.D / IG_TZ, d.N);
  const dim3 grid((unsigned)tiles_xy, (unsigned)(d.D / IG_TZ), (unsigned)d.N);
  SEUNET_DTYPE_SWITCH(dtype, {
    if (ce == 8) return input_grad_ic<T, 8>(draw, w_ec1, x0, in_channel, gx0, gx1, grad_x, d, grid, s);
    return input_grad_ic<T, 16>(draw, w_ec1, x0, in_channel, gx0, gx1, grad_x, d, grid, s);
  });
  return 0;
}

}  // namespace seunet
