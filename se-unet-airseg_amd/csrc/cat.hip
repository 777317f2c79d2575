// The aggregation block (reference CATConv, SE_UNet.py:45-49, and the residual adds at :187,196,205):
//     raw -> InstanceNorm -> LeakyReLU (+ the same for a second branch, added)
// and its backward (two-phase InstanceNorm backward).  Thread mapping and the steps shared with gate.hip: epilogue.h.
// The "x" branch of an encoder aggregation block (a 1x1x1 conv of the <= 2-channel network input) is recomputed per voxel
// instead of read, its statistics come from the input's second moments, and its weight gradient is formed from sums of the
// backward pass A (XR / XW template modes below).
#include "epilogue.h"
#include "wgrad.h"
#include <type_traits>

namespace seunet {

// ---- aggregation block (1x1x1 conv output -> IN -> LeakyReLU, optional second branch added) ------------------------------
// XR (x-branch recompute): the second branch is the 1x1x1 conv of the <= 2-channel network input (x33 / x63 / x93,
//     SE_UNet.py:112,118,124).  Its raw output is never stored: `raw2` then points at the packed 8-channel INPUT
//     [N][V][8] and raw2[c] = w2x[c][0]*x0 + w2x[c][1]*x1 is recomputed per voxel (16 B read instead of 2C bytes);
//     its InstanceNorm statistics come from the input's second moments (xbranch_stats_kernel).
template <bool XR>
__device__ __forceinline__ void second_branch(const float (&in8)[8], const float (&wa)[8], const float (&wb)[8], float (&x2)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) x2[j] = XR ? wa[j] * in8[0] + wb[j] * in8[1] : in8[j];
}

template <typename T, int LPV, bool TWO, bool XR>
__global__ void __launch_bounds__(EPI_THREADS)
cat_fwd_kernel(const T* __restrict__ raw, const float* __restrict__ mean, const float* __restrict__ rstd,
               const T* __restrict__ raw2, const float* __restrict__ mean2, const float* __restrict__ rstd2, int C, float slope,
               T* __restrict__ out, long long V, const float* __restrict__ w2x, int xic) {
  SEUNET_EPI_THREAD(LPV);
  float mu[8], rs[8], mu2[8], rs2[8], wa[8], wb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = mean[n * C + c0 + j]; rs[j] = rstd[n * C + c0 + j];
    mu2[j] = TWO ? mean2[n * C + c0 + j] : 0.f;
    rs2[j] = TWO ? rstd2[n * C + c0 + j] : 0.f;
    wa[j] = XR ? w2x[(c0 + j) * xic] : 0.f;
    wb[j] = (XR && xic > 1) ? w2x[(c0 + j) * xic + 1] : 0.f;
  }
  const long long stride = (long long)P * VPB;
  long long v = (long long)blockIdx.x * VPB + vb;
  Pack8<T> nx, nx2;   // software pipeline: voxel v + stride is loaded before voxel v is computed
  zero8p(nx); zero8p(nx2);
  if (v < V) {
    const long long o = ((long long)n * V + v) * C + c0;
    load8p(raw + o, nx);
    if (TWO) load8p(XR ? raw2 + ((long long)n * V + v) * 8 : raw2 + o, nx2);
  }
  for (; v < V; v += stride) {
    const long long o = ((long long)n * V + v) * C + c0;
    float x[8], in2[8], x2[8], y[8];
    unpack8(nx, x);
    if (TWO) { unpack8(nx2, in2); second_branch<XR>(in2, wa, wb, x2); }
    if (v + stride < V) {
      load8p(raw + o + stride * C, nx);
      if (TWO) load8p(XR ? raw2 + ((long long)n * V + v + stride) * 8 : raw2 + o + stride * C, nx2);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = norm_lrelu(x[j], mu[j], rs[j], slope);
    if (TWO) {
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] += norm_lrelu(x2[j], mu2[j], rs2[j], slope);
    }
    store8(out + o, y);
  }
}

// The aggregation block's forward with the 2x2x2 max-pool that follows it in the encoder (SE_UNet.py:188-189, 197-198,
// 206-207: ec33 -> pool0, ec63 -> pool1, ec93 -> pool2) written by the same kernel: a thread owns one pooling window x 8
// channels, computes the block output of its eight voxels (norm_lrelu of both branches, as cat_fwd_kernel<.., true, true>
// does), stores them and their maximum.  The pooled tensor costs one extra 1/8-size store instead of a second read of the
// full-resolution output.
// (Rounding is monotonic, so the maximum of the rounded values the separate kernel reads equals the rounded maximum.)
template <typename T, int LPV>
__global__ void __launch_bounds__(EPI_THREADS)
cat_fwd_pool_kernel(const T* __restrict__ raw, const float* __restrict__ mean, const float* __restrict__ rstd,
                    const T* __restrict__ xin, const float* __restrict__ mean2, const float* __restrict__ rstd2, int C, float slope,
                    T* __restrict__ out, T* __restrict__ pooled, int D, int H, int W, const float* __restrict__ w2x, int xic,
                    unsigned* __restrict__ argmax) {
  SEUNET_EPI_THREAD(LPV);
  float mu[8], rs[8], mu2[8], rs2[8], wa[8], wb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = mean[n * C + c0 + j]; rs[j] = rstd[n * C + c0 + j];
    mu2[j] = mean2[n * C + c0 + j]; rs2[j] = rstd2[n * C + c0 + j];
    wa[j] = w2x[(c0 + j) * xic];
    wb[j] = xic > 1 ? w2x[(c0 + j) * xic + 1] : 0.f;
  }
  const int Do = D / 2, Ho = H / 2, Wo = W / 2;
  const long long V = (long long)D * H * W, Vo = (long long)Do * Ho * Wo;
  const long long stride = (long long)P * VPB;
  for (long long cv = (long long)blockIdx.x * VPB + vb; cv < Vo; cv += stride) {
    const int xo = (int)(cv % Wo);
    const int yo = (int)((cv / Wo) % Ho);
    const int zo = (int)(cv / ((long long)Wo * Ho));
    const long long v0 = ((long long)(2 * zo) * H + 2 * yo) * W + 2 * xo;
    Pack8<T> px[8], pi[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {   // all sixteen loads of the window in flight
      const long long v = v0 + ((long long)(k >> 2) * H + ((k >> 1) & 1)) * W + (k & 1);
      load8p(raw + ((long long)n * V + v) * C + c0, px[k]);
      load8p(xin + ((long long)n * V + v) * 8, pi[k]);
    }
    float m[8];
    unsigned am = 0;      // 3 bits per channel: the window position (z, y, x scan order) of the FIRST maximum of the STORED values
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const long long v = v0 + ((long long)(k >> 2) * H + ((k >> 1) & 1)) * W + (k & 1);
      float x[8], in2[8], x2[8], y[8];
      unpack8(px[k], x);
      unpack8(pi[k], in2);
      second_branch<true>(in2, wa, wb, x2);
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = norm_lrelu(x[j], mu[j], rs[j], slope);
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] += norm_lrelu(x2[j], mu2[j], rs2[j], slope);
      store8(out + ((long long)n * V + v) * C + c0, y);
      // the maximum (and its position) of the values as stored: what a max-pool over the stored tensor sees (two different f32
      // values may round to the same 16-bit value; the reference's first-maximum rule then picks the earlier one)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float yr = round_to<T>(y[j]);
        if (yr > m[j]) { m[j] = yr; am = (am & ~(7u << (3 * j))) | ((unsigned)k << (3 * j)); }
      }
    }
    store8(pooled + ((long long)n * Vo + cv) * C + c0, m);
    if (argmax != nullptr) argmax[((long long)n * Vo + cv) * (C / 8) + cg] = am;
  }
}

// The gradient that arrives through the 2x2x2 max-pool consuming this block's output (encoder: ec33 -> pool0, ec63 -> pool1,
// ec93 -> pool2) is added ON THE FLY in both passes instead of being scattered into g_out by a pooling-backward kernel first
// (a read-modify-write of the whole full-resolution gradient): window word of arg-max positions (cat_fwd_pool_kernel) + the
// pooled gradient, 20 bytes per voxel and 8 channels, shared by the eight voxels of a window through the caches.
struct PoolRef {
  const unsigned* argmax;     // [N][Vo][C/8], 3 bits per channel; null = no pool gradient
  const void* g_pool;         // [N][Vo][C]
  unsigned W, H, Wo, Ho;      // extents of THIS block's level, and of the pooled level
  unsigned mW, mH;            // floor(2^32 / W), floor(2^32 / H)
  long long Vo;
};
__device__ __forceinline__ unsigned div_small(unsigned n, unsigned d, unsigned m, unsigned& rem) {
  unsigned q = __umulhi(n, m);            // q <= n / d <= q + 1
  unsigned r = n - q * d;
  if (r >= d) { ++q; r -= d; }
  rem = r;
  return q;
}
// window position (0..7, z-y-x scan order) of voxel v and the index of its window
__device__ __forceinline__ void pool_locate(const PoolRef& pr, unsigned v, unsigned& kpos, unsigned& cv) {
  unsigned x, y;
  const unsigned t = div_small(v, pr.W, pr.mW, x);
  const unsigned z = div_small(t, pr.H, pr.mH, y);
  kpos = ((z & 1u) << 2) | ((y & 1u) << 1) | (x & 1u);
  cv = ((z >> 1) * pr.Ho + (y >> 1)) * pr.Wo + (x >> 1);
}

// APPLY = false: per-(n,c) f64 sums of dxhat, dxhat*xhat for one or two branches (nothing stored)
// APPLY = true : draw = rstd * (dxhat - m1 - xhat * m2) for each branch (dxhat_out may alias g_out)
// XW (pass A of a two-branch block whose second branch is a 1x1x1 conv of the <= 2-channel network input, the x33 / x63 /
//     x93 detail-injection convs): that conv's weight gradient dW2[c][i] = sum_v draw2[v][c] * x[v][i] is NOT accumulated
//     from draw2.  sum_v draw2 = 0 and sum_v draw2 * xhat2 = 0, and xhat2 is itself linear in x, so the sum is what is left of
//     O(1) terms that cancel to ~1e-5 of their size at 128^3; formed from the f32 draw2 (f32 m1 / m2 / mean / rstd, each a
//     systematic offset times the voxel count) it was 4.6e-2 off at 1 x 128^3 in fp32 mode -- and so is the fp32 reference.
//     Instead pass A also sums S_i[c] = sum_v dxhat2[v][c] * x_i[v] (dxhat2 = g * LeakyReLU'; one record per block), and
//     xw_finalize_kernel forms the gradient in f64 from S_i, sum_v dxhat2 and the input's first / second moments.
// XG (pass B of an XR block, only when the network input's gradient is requested): each lane also contracts its eight draw2
//     values with the x-branch weight, p_k = sum_j draw2[c0 + j] * W2[c0 + j][k] (k < in_channel), the LPV lanes of the voxel add
//     their p_k in a fixed butterfly order and lane 0 writes (or adds to) gx_out [N][V][in_channel] f32 -- the x-branch's
//     contribution W2^T draw2 to the input gradient at this level (net.cpp, seunet_net_backward_input).
template <typename T, int LPV, bool TWO, bool APPLY, bool XW, bool XR, bool XG>
__global__ void __launch_bounds__(EPI_THREADS)
cat_bwd_kernel(const T* g_out, const T* __restrict__ raw, const float* __restrict__ mean, const float* __restrict__ rstd,
               const T* __restrict__ raw2, const float* __restrict__ mean2, const float* __restrict__ rstd2, int C, float slope,
               const float* __restrict__ m1p, const float* __restrict__ m2p, const float* __restrict__ m1bp,
               const float* __restrict__ m2bp, T* dxhat_out, T* dxhat2_out, double* __restrict__ stat_partial,
               double* __restrict__ stat_partial2, long long V, double* __restrict__ xw_partial, const float* __restrict__ w2x,
               int xic, PoolRef pool, float* __restrict__ gx_out, int gx_acc) {
  static_assert(!XG || (APPLY && XR), "XG: pass B of an XR block only");
  static_assert(!XW || XR, "XW: the weight-gradient sums are formed from the recomputed branch's own input voxel");
  SEUNET_EPI_THREAD(LPV);
  const bool pooled = pool.argmax != nullptr;                       // (uniform)
  const unsigned* pam = pool.argmax + (long long)n * pool.Vo * (C / 8) + cg;
  const T* pgp = reinterpret_cast<const T*>(pool.g_pool) + (long long)n * pool.Vo * C + c0;
  float mu[8], rs[8], mu2[8], rs2[8], a1[8], a2[8], b1[8], b2[8];
  typedef typename std::conditional<sizeof(T) == 2, float, double>::type SumT;   // (bf16: f32 thread sums, see sse_bwd_kernel)
  SumT s[4][8];
  SumT xw[8][2];
  float wa[8], wb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    xw[j][0] = xw[j][1] = 0.0;
    wa[j] = XR ? w2x[(c0 + j) * xic] : 0.f;
    wb[j] = (XR && xic > 1) ? w2x[(c0 + j) * xic + 1] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = mean[n * C + c0 + j]; rs[j] = rstd[n * C + c0 + j];
    mu2[j] = TWO ? mean2[n * C + c0 + j] : 0.f;
    rs2[j] = TWO ? rstd2[n * C + c0 + j] : 0.f;
    a1[j] = APPLY ? m1p[n * C + c0 + j] : 0.f;
    a2[j] = APPLY ? m2p[n * C + c0 + j] : 0.f;
    b1[j] = (APPLY && TWO) ? m1bp[n * C + c0 + j] : 0.f;
    b2[j] = (APPLY && TWO) ? m2bp[n * C + c0 + j] : 0.f;
    s[0][j] = s[1][j] = s[2][j] = s[3][j] = 0.0;
  }
  const long long stride = (long long)P * VPB;
  long long v = (long long)blockIdx.x * VPB + vb;
  Pack8<T> ng, nx, nx2, npg;   // software pipeline: voxel v + stride is loaded before voxel v is computed
  unsigned nam = 0, nkpos = 0;
  zero8p(ng); zero8p(nx); zero8p(nx2); zero8p(npg);
  auto fetch_pool = [&](long long vv) __attribute__((always_inline)) {
    unsigned cv;
    pool_locate(pool, (unsigned)vv, nkpos, cv);
    nam = pam[(long long)cv * (C / 8)];
    load8p(pgp + (long long)cv * C, npg);
  };
  if (v < V) {
    const long long o = ((long long)n * V + v) * C + c0;
    load8p(g_out + o, ng);
    load8p(raw + o, nx);
    if (TWO) load8p(XR ? raw2 + ((long long)n * V + v) * 8 : raw2 + o, nx2);
    if (pooled) fetch_pool(v);
  }
  for (; v < V; v += stride) {
    const long long o = ((long long)n * V + v) * C + c0;
    float gy[8], x[8], in2[8], x2[8], d[8];
    unpack8(ng, gy);
    unpack8(nx, x);
    if (TWO) { unpack8(nx2, in2); second_branch<XR>(in2, wa, wb, x2); }
    if (pooled) {           // + the pooled gradient where this voxel was its window's maximum
      float gp[8];
      unpack8(npg, gp);
#pragma unroll
      for (int j = 0; j < 8; ++j) gy[j] += ((nam >> (3 * j)) & 7u) == nkpos ? gp[j] : 0.f;
    }
    if (v + stride < V) {   // a later voxel of this same thread: never written by anyone before it is read
      load8p(g_out + o + stride * C, ng);
      load8p(raw + o + stride * C, nx);
      if (TWO) load8p(XR ? raw2 + ((long long)n * V + v + stride) * 8 : raw2 + o + stride * C, nx2);
      if (pooled) fetch_pool(v + stride);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xh = (x[j] - mu[j]) * rs[j];
      d[j] = gy[j] * lrelu_slope(xh, slope);
      if (APPLY) d[j] = rs[j] * (d[j] - a1[j] - xh * a2[j]);
      else { s[0][j] += (SumT)d[j]; s[1][j] += (SumT)d[j] * (SumT)xh; }
    }
    if (TWO) {
      float d2[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xh = (x2[j] - mu2[j]) * rs2[j];
        d2[j] = gy[j] * lrelu_slope(xh, slope);
        if (APPLY) d2[j] = rs2[j] * (d2[j] - b1[j] - xh * b2[j]);
        else { s[2][j] += (SumT)d2[j]; s[3][j] += (SumT)d2[j] * (SumT)xh; }
      }
      if (APPLY && !XR) store8(dxhat2_out + o, d2);
      if (XG) {
        float pa = 0.f, pb = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { pa = fmaf(d2[j], wa[j], pa); pb = fmaf(d2[j], wb[j], pb); }
        // (the LPV lanes of one voxel share v: all active or all inactive together; the shuffles stay inside the group)
#pragma unroll
        for (int off = 1; off < LPV; off <<= 1) { pa += shfl_xor_settled(pa, off); pb += shfl_xor_settled(pb, off); }
        if (cg == 0) {
          float* gp = gx_out + ((long long)n * V + v) * xic;
          gp[0] = gx_acc ? gp[0] + pa : pa;
          if (xic > 1) gp[1] = gx_acc ? gp[1] + pb : pb;
        }
      }
      if (XW && !APPLY) {   // (in2: the packed 8-channel input voxel of the recomputed branch)
#pragma unroll
        for (int j = 0; j < 8; ++j) { xw[j][0] += (SumT)d2[j] * (SumT)in2[0]; xw[j][1] += (SumT)d2[j] * (SumT)in2[1]; }
      }
    }
    if (APPLY) store8(dxhat_out + o, d);  // may alias g_out (same element, read before write)
  }
  if (APPLY) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // (the wave-order sums below are wave4_sum spelled out: as calls they changed the schedule of twelve pass-A instantiations)
  if (XW) {   // block record [C][2] (f64), fixed-order sums
    __shared__ double redx[4][16][16];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const double r = stride_sum_d<LPV>((double)xw[j][i]);
        if (lane < LPV) redx[wave][lane][j * 2 + i] = r;
      }
    __syncthreads();
    double* rec = xw_partial + ((long long)n * P + blockIdx.x) * (C * 2);
    for (int e = threadIdx.x; e < LPV * 16; e += EPI_THREADS) {
      const int gq = e / 16, k = e % 16;
      rec[(gq * 8 + (k >> 1)) * 2 + (k & 1)] = ((redx[0][gq][k] + redx[1][gq][k]) + redx[2][gq][k]) + redx[3][gq][k];
    }
  }
  __shared__ double red[4][16][32];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const double r = stride_sum_d<LPV>((double)s[q][j]);
      if (lane < LPV) red[wave][lane][q * 8 + j] = r;
    }
  __syncthreads();
  const long long rec = (long long)n * P + blockIdx.x;
  for (int i = threadIdx.x; i < LPV * 32; i += EPI_THREADS) {
    const int gq = i / 32, k = i % 32, q = k >> 3;
    const double tot = ((red[0][gq][k] + red[1][gq][k]) + red[2][gq][k]) + red[3][gq][k];
    const int c = gq * 8 + (k & 7);
    if (q < 2) stat_partial[(rec * C + c) * 2 + q] = tot;
    else if (TWO) stat_partial2[(rec * C + c) * 2 + (q - 2)] = tot;
  }
}

// ----------------------------------------------------------------------------------
// x-branch statistics without the x-branch tensor.  raw2 = W2 x is linear in the (<= 2-channel) input, so its per-(n,c)
// InstanceNorm statistics follow from the input's first and second moments per sample:
//     mean2[c] = sum_i W2[c][i] m_i,      var2[c] = sum_ij W2[c][i] W2[c][j] (M_ij - m_i m_j)        (f64)
// ----------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(EPI_THREADS)
input_moments_kernel(const T* __restrict__ xin, double* __restrict__ partial, long long V) {
  const int n = blockIdx.y, P = gridDim.x;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // x0, x1, x0^2, x0 x1, x1^2
  for (long long v = (long long)blockIdx.x * EPI_THREADS + threadIdx.x; v < V; v += (long long)P * EPI_THREADS) {
    float x[8];
    load8(xin + ((long long)n * V + v) * 8, x);
    const double a = (double)x[0], b = (double)x[1];
    s[0] += a; s[1] += b; s[2] += a * a; s[3] += a * b; s[4] += b * b;
  }
  __shared__ double red[4][5];
  block_sum(s, red);
  if (const int k = threadIdx.x; k < 5) partial[((long long)n * P + blockIdx.x) * 5 + k] = wave4_sum(red, k);
}

// one 256-thread block per sample: fixed-order sum of the moment partials, then mean / rstd of every output channel
__global__ void __launch_bounds__(256)
xbranch_stats_kernel(const double* __restrict__ partial, int slots, const float* __restrict__ w2, int C, int ic,
                     double inv_count, float eps, float* __restrict__ mean2, float* __restrict__ rstd2,
                     double* __restrict__ moments_out) {
  const int n = blockIdx.x;
  __shared__ double red[4][5], tot[5];
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < slots; b += 256)
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k] += partial[((long long)n * slots + b) * 5 + k];
  block_sum(s, red);
  if (threadIdx.x < 5) tot[threadIdx.x] = wave4_sum(red, threadIdx.x) * inv_count;
  __syncthreads();
  // (kept for the backward pass: the x-branch weight gradient is formed from these and two sums per channel, xw_finalize_kernel)
  if (moments_out != nullptr && threadIdx.x < 5) moments_out[n * 5 + threadIdx.x] = tot[threadIdx.x];
  const double m0 = tot[0], m1 = tot[1];
  const double c00 = tot[2] - m0 * m0, c01 = tot[3] - m0 * m1, c11 = tot[4] - m1 * m1;
  for (int c = threadIdx.x; c < C; c += 256) {
    const double a = (double)w2[c * ic], b = ic > 1 ? (double)w2[c * ic + 1] : 0.0;
    const double mu = a * m0 + b * m1;
    double var = a * a * c00 + 2.0 * a * b * c01 + b * b * c11;
    if (var < 0.0) var = 0.0;
    mean2[n * C + c] = (float)mu;
    rstd2[n * C + c] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

// dW2 (PyTorch layout (C, in_channel, 1, 1, 1)) of an x-branch conv, in f64 from sums (cat_bwd_kernel XW).  Per sample, with
// xc_k = x_k - mean(x_k), Cov = the input's 2 x 2 covariance (per-voxel mean), xhat2 = rs * sum_k w_k xc_k, rs^2 = 1 / (w' Cov w
// + eps), dxhat2 = g * LeakyReLU'(xhat2) and A_k = sum_v dxhat2 xc_k = S_k - mean(x_k) * sum_v dxhat2:
//     draw2 = rs * (dxhat2 - mean(dxhat2) - xhat2 * mean(dxhat2 * xhat2))             (InstanceNorm backward)
//     dW2_i = sum_v draw2 * x_i = rs * (A_i - rs^2 * (sum_k w_k A_k) * (sum_k w_k Cov_ki))
// (the mean(dxhat2) term drops out against sum_v xc_i = 0).  The cancellation between A_i and its projection on w happens in
// f64 here; the f32 inputs of the sums (dxhat2 = g or slope * g, x) enter only through products that are exact in f64.
// One block per output channel; fixed summation order (slots within a sample, then samples): bitwise reproducible.
__device__ __forceinline__ void
xw_finalize_body(int c, const double* __restrict__ xw_partial, const double* __restrict__ stat_partial2, int slots, int C, int N,
                 const double* __restrict__ moments, const float* __restrict__ w2, int ic, double eps, float* __restrict__ dw) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __shared__ double red[4][3];
  const double wa = (double)w2[c * ic], wb = ic > 1 ? (double)w2[c * ic + 1] : 0.0;
  double g0 = 0.0, g1 = 0.0;
  for (int n = 0; n < N; ++n) {
    double s[3] = {0.0, 0.0, 0.0};       // S_0, S_1, sum dxhat2
    for (int r = threadIdx.x; r < slots; r += 256) {
      const long long rec = (long long)n * slots + r;
      s[0] += xw_partial[(rec * C + c) * 2 + 0];
      s[1] += xw_partial[(rec * C + c) * 2 + 1];
      s[2] += stat_partial2[(rec * C + c) * 2 + 0];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {   // (block_sum spelled out: as a call inside the sample loop it changed this kernel's code)
      double r = s[k];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) r += shfl_xor_settled(r, off);
      if (lane == 0) red[wave][k] = r;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const double S0 = wave4_sum(red, 0), S1 = wave4_sum(red, 1), Sd = wave4_sum(red, 2);
      const double* m = moments + n * 5;      // mean x0, mean x1, mean x0^2, mean x0 x1, mean x1^2
      const double c00 = m[2] - m[0] * m[0], c01 = m[3] - m[0] * m[1], c11 = m[4] - m[1] * m[1];
      const double A0 = S0 - m[0] * Sd, A1 = S1 - m[1] * Sd;
      double var = wa * wa * c00 + 2.0 * wa * wb * c01 + wb * wb * c11;
      if (var < 0.0) var = 0.0;
      const double rs2 = 1.0 / (var + eps), rs = sqrt(rs2);
      const double proj = wa * A0 + wb * A1;
      g0 += rs * (A0 - rs2 * proj * (wa * c00 + wb * c01));
      g1 += rs * (A1 - rs2 * proj * (wa * c01 + wb * c11));
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    dw[c * ic] = (float)g0;
    if (ic > 1) dw[c * ic + 1] = (float)g1;
  }
}
__global__ void __launch_bounds__(256)
xw_finalize_kernel(const double* __restrict__ xw_partial, const double* __restrict__ stat_partial2, int slots, int C, int N,
                   const double* __restrict__ moments, const float* __restrict__ w2, int ic, double eps, float* __restrict__ dw) {
  xw_finalize_body(blockIdx.x, xw_partial, stat_partial2, slots, C, N, moments, w2, ic, eps, dw);
}
// what follows pass A of an aggregation block, in ONE launch (the gated block's gate_bwd_finalize_kernel is the model): blocks
// [0, N*C) the first branch's two means, the next nb2 = N*C or 0 the second branch's, the next nxw = C or 0 the recomputed
// x-branch's weight gradient, and any blocks past those the rider (wgrad.h).  Pass B waits for the means alone: they come first.
__global__ void __launch_bounds__(256)
cat_bwd_finalize_kernel(const double* __restrict__ partial, const double* __restrict__ partial2, int slots, int C, int N,
                        double inv_count, float* __restrict__ m1, float* __restrict__ m2, float* __restrict__ m1b,
                        float* __restrict__ m2b, int nb2, int nxw, const double* __restrict__ xw_partial,
                        const double* __restrict__ moments, const float* __restrict__ w2, int ic, double eps, float* __restrict__ dw,
                        WgReduceJob rider) {
  const int b = blockIdx.x, nb = N * C;
  if (b < nb) stats_finalize_body(b, partial, slots, C, inv_count, 0.f, 1, m1, m2);
  else if (b < nb + nb2) stats_finalize_body(b - nb, partial2, slots, C, inv_count, 0.f, 1, m1b, m2b);
  else if (b < nb + nb2 + nxw) xw_finalize_body(b - nb - nb2, xw_partial, partial2, slots, C, N, moments, w2, ic, eps, dw);
  else wgrad_reduce_body(rider, b - nb - nb2 - nxw);
}

// diagnostic (seunet_net_read_tensor): the x-branch's raw values, recomputed by the same device function as the aggregation
// epilogue uses (second_branch<true>: same expression, same contraction), written as NCDHW f32
template <typename T>
__global__ void __launch_bounds__(256)
xbranch_values_kernel(const T* __restrict__ x_in, const float* __restrict__ w2x, int C, int xic, float* __restrict__ out, long long V,
                      long long total) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int cg = (int)(i % (C / 8));
    const long long nv = i / (C / 8);           // n * V + v
    const long long n = nv / V, v = nv % V;
    float wa[8], wb[8], in2[8], x2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      wa[j] = w2x[(cg * 8 + j) * xic];
      wb[j] = xic > 1 ? w2x[(cg * 8 + j) * xic + 1] : 0.f;
    }
    Pack8<T> px;
    load8p(x_in + nv * 8, px);
    unpack8(px, in2);
    second_branch<true>(in2, wa, wb, x2);
#pragma unroll
    for (int j = 0; j < 8; ++j) out[(n * C + cg * 8 + j) * V + v] = x2[j];
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
// What every launcher of the block starts with: the channel check and the second branch as the kernels take it (x: all null
// for Branch2::None), with its in_channel check; `who` names the entry point.
static int cat_branch(const char* who, const CatBlock& b, Branch2& x, bool& two, bool& xr) {
  if (int e = check_c(b.C)) return e;
  x = b.b.kind == Branch2::None ? Branch2{} : b.b;
  two = x.kind != Branch2::None;
  xr = x.kind == Branch2::Recomputed;
  SEUNET_CHECK(!xr || (x.in_channel >= 1 && x.in_channel <= 2), "%s: in_channel %d (1 or 2)", who, x.in_channel);
  return 0;
}

int launch_cat_fwd(int dtype, const CatBlock& b, void* out, const PoolOut& pool, Dims d, hipStream_t s) {
  Branch2 x;
  bool two, xr;
  if (int e = cat_branch("cat_epilogue_fwd", b, x, two, xr)) return e;
  SEUNET_CHECK(!pool.pooled || (xr && d.D % 2 == 0 && d.H % 2 == 0 && d.W % 2 == 0),
               "cat_epilogue_fwd: the fused max-pool needs a recomputed second branch and even extents");
  dim3 grid(epi_partials(d) * 4, d.N);
#define SEUNET_CAT_FWD(...) <<<grid, EPI_THREADS, 0, s>>>((const T*)b.a.raw, b.a.mean, b.a.rstd, (const T*)x.src, x.mean2, x.rstd2, b.C, b.slope, (T*)out, __VA_ARGS__)
  SEUNET_LPV_SWITCH(b.C / 8, {
    SEUNET_DTYPE_SWITCH(dtype, {
      if (pool.pooled) cat_fwd_pool_kernel<T, LPV> SEUNET_CAT_FWD((T*)pool.pooled, d.D, d.H, d.W, x.w2, x.in_channel, pool.argmax);
      else if (xr) cat_fwd_kernel<T, LPV, true, true> SEUNET_CAT_FWD(d.vox(), x.w2, x.in_channel);
      else if (two) cat_fwd_kernel<T, LPV, true, false> SEUNET_CAT_FWD(d.vox(), nullptr, 0);
      else cat_fwd_kernel<T, LPV, false, false> SEUNET_CAT_FWD(d.vox(), nullptr, 0);
    });
  });
#undef SEUNET_CAT_FWD
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// the host side of PoolRef, with what both backward passes check of it
static int cat_bwd_pool(const char* who, bool xr, const PoolGrad& pool, Dims d, PoolRef& pr) {
  pr = PoolRef{};
  if (pool.argmax == nullptr) return 0;
  SEUNET_CHECK(xr && pool.g_pool != nullptr && d.D % 2 == 0 && d.H % 2 == 0 && d.W % 2 == 0 && d.vox() < (1ll << 31),
               "%s: pooled gradient needs a recomputed second branch and even extents below 2^31 voxels", who);
  pr.argmax = pool.argmax; pr.g_pool = pool.g_pool;
  pr.W = (unsigned)d.W; pr.H = (unsigned)d.H; pr.Wo = (unsigned)d.W / 2; pr.Ho = (unsigned)d.H / 2;
  pr.mW = (unsigned)((1ull << 32) / (unsigned)d.W); pr.mH = (unsigned)((1ull << 32) / (unsigned)d.H);
  pr.Vo = d.vox() / 8;
  return 0;
}

// one argument list for every instantiation: x is the second branch (all null for Branch2::None), o / a the pass's own struct
// and a null one for the other pass
#define SEUNET_CAT_BWD(TWO, APPLY, XW, XR, XG)                                                                                   \
  cat_bwd_kernel<T, LPV, TWO, APPLY, XW, XR, XG><<<grid, EPI_THREADS, 0, s>>>(                                                    \
      (const T*)g_out, (const T*)b.a.raw, b.a.mean, b.a.rstd, (const T*)x.src, x.mean2, x.rstd2, b.C, b.slope, a.m1, a.m2, a.m1b, \
      a.m2b, (T*)a.dx, (T*)a.dx2, o.stat_partial, o.stat_partial2, d.vox(), o.xw_partial, x.w2, x.in_channel, pr, a.gx_out,     \
      a.gx_acc)

int launch_cat_bwd_sums(int dtype, const CatBlock& b, const void* g_out, const PoolGrad& pool, const CatSums& out, Dims d,
                        hipStream_t s) {
  Branch2 x;
  bool two, xr;
  PoolRef pr;
  if (int e = cat_branch("cat_epilogue_bwd_sums", b, x, two, xr)) return e;
  if (int e = cat_bwd_pool("cat_epilogue_bwd_sums", xr, pool, d, pr)) return e;
  SEUNET_CHECK(out.stat_partial && (!two || out.stat_partial2), "cat_epilogue_bwd_sums needs the partial buffers");
  SEUNET_CHECK(!out.xw_partial || xr, "cat_epilogue_bwd_sums: the weight-gradient sums belong to a recomputed second branch");
  const CatSums o{out.stat_partial, two ? out.stat_partial2 : nullptr, out.xw_partial};
  const CatApply a{};
  dim3 grid(epi_partials(d), d.N);
  SEUNET_LPV_SWITCH(b.C / 8, {
    SEUNET_DTYPE_SWITCH(dtype, {
      if (xr && o.xw_partial) SEUNET_CAT_BWD(true, false, true, true, false);
      else if (xr) SEUNET_CAT_BWD(true, false, false, true, false);
      else if (two) SEUNET_CAT_BWD(true, false, false, false, false);
      else SEUNET_CAT_BWD(false, false, false, false, false);
    });
  });
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_cat_bwd_apply(int dtype, const CatBlock& b, const void* g_out, const PoolGrad& pool, const CatApply& io, Dims d,
                         hipStream_t s) {
  Branch2 x;
  bool two, xr;
  PoolRef pr;
  if (int e = cat_branch("cat_epilogue_bwd_apply", b, x, two, xr)) return e;
  if (int e = cat_bwd_pool("cat_epilogue_bwd_apply", xr, pool, d, pr)) return e;
  SEUNET_CHECK(io.m1 && io.m2 && io.dx && (!two || (io.m1b && io.m2b)) && (!two || xr || io.dx2),
               "cat_epilogue_bwd_apply: missing argument");
  SEUNET_CHECK(!io.gx_out || xr, "cat_epilogue_bwd_apply: the input-gradient term belongs to a recomputed second branch");
  const CatApply a{io.m1, io.m2, two ? io.m1b : nullptr, two ? io.m2b : nullptr, io.dx, two && !xr ? io.dx2 : nullptr,
                   io.gx_out, io.gx_out ? io.gx_acc : 0};
  const CatSums o{};
  dim3 grid(epi_partials(d) * 4, d.N);
  SEUNET_LPV_SWITCH(b.C / 8, {
    SEUNET_DTYPE_SWITCH(dtype, {
      if (xr && a.gx_out) SEUNET_CAT_BWD(true, true, false, true, true);
      else if (xr) SEUNET_CAT_BWD(true, true, false, true, false);
      else if (two) SEUNET_CAT_BWD(true, true, false, false, false);
      else SEUNET_CAT_BWD(false, true, false, false, false);
    });
  });
  SEUNET_LAUNCH_CHECK();
  return 0;
}
#undef SEUNET_CAT_BWD

// ---- the x-branch (XR): moments, statistics, weight gradient, diagnostic values ------------------------------------------
int xbranch_moment_slots(Dims d) { return epi_partials(d); }

int launch_xbranch_moments(int dtype, const void* x_in, double* partial, Dims d, hipStream_t s) {
  dim3 grid(xbranch_moment_slots(d), d.N);
  SEUNET_DTYPE_SWITCH(dtype, input_moments_kernel<T><<<grid, EPI_THREADS, 0, s>>>((const T*)x_in, partial, d.vox()));
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_xbranch_stats(const double* partial, int slots, const float* w2, int C, int in_channel, int N, long long count,
                         float eps, float* mean2, float* rstd2, double* moments_out, hipStream_t s) {
  SEUNET_CHECK(in_channel >= 1 && in_channel <= 2, "xbranch_stats: in_channel %d (1 or 2)", in_channel);
  xbranch_stats_kernel<<<N, 256, 0, s>>>(partial, slots, w2, C, in_channel, 1.0 / (double)count, eps, mean2, rstd2, moments_out);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_cat_xgrad_finalize(const double* xw_partial, const double* stat_partial2, int slots, const double* moments, const float* w2,
                              int C, int in_channel, int N, float eps, float* dw, hipStream_t s) {
  SEUNET_CHECK(in_channel >= 1 && in_channel <= 2, "cat_xgrad_finalize: in_channel %d (1 or 2)", in_channel);
  xw_finalize_kernel<<<C, 256, 0, s>>>(xw_partial, stat_partial2, slots, C, N, moments, w2, in_channel, (double)eps, dw);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_cat_bwd_finalize(const double* stat_partial, const double* stat_partial2, int slots, int C, int N, long long count,
                            float* m1, float* m2, float* m1b, float* m2b, const CatXwFinalize& xw, hipStream_t s,
                            const WgReduceJob* rider) {
  SEUNET_CHECK(stat_partial && m1 && m2 && (!stat_partial2 || (m1b && m2b)), "cat_bwd_finalize: missing argument");
  SEUNET_CHECK(!xw.dw || (stat_partial2 && xw.xw_partial && xw.moments && xw.w2 && xw.in_channel >= 1 && xw.in_channel <= 2),
               "cat_bwd_finalize: the x-branch weight gradient needs the second branch's sums and in_channel 1 or 2");
  const WgReduceJob job = rider ? *rider : WgReduceJob{};
  const int nb2 = stat_partial2 ? N * C : 0, nxw = xw.dw ? C : 0;
  cat_bwd_finalize_kernel<<<N * C + nb2 + nxw + job.blocks(), 256, 0, s>>>(
      stat_partial, stat_partial2, slots, C, N, 1.0 / (double)count, m1, m2, m1b, m2b, nb2, nxw, xw.xw_partial, xw.moments, xw.w2,
      xw.in_channel, (double)xw.eps, xw.dw, job);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_xbranch_values(int dtype, const void* x_in, const float* w2, int C, int in_channel, float* out, Dims d, hipStream_t s) {
  SEUNET_CHECK(in_channel >= 1 && in_channel <= 2 && C % 8 == 0, "xbranch_values: bad argument");
  const long long total = (long long)d.N * d.vox() * (C / 8);
  const int grid = (int)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
  SEUNET_DTYPE_SWITCH(dtype, xbranch_values_kernel<T><<<grid, 256, 0, s>>>((const T*)x_in, w2, C, in_channel, out, d.vox(), total));
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
