// The gated block (reference SSEConv / SSEConv2, SE_UNet.py:24-35, 68-82):
//     raw conv output -> InstanceNorm -> LeakyReLU -> spatial gate(s) -> e ; side = conv1x1(e)
// and its backward (two-phase InstanceNorm backward).  Thread mapping and the steps shared with cat.hip: epilogue.h.
#include "epilogue.h"
#include "wgrad.h"

namespace seunet {

// ---- gated block, forward ------------------------------------------------------------------------------------------------
template <typename T, int LPV, bool G2>
__global__ void __launch_bounds__(EPI_THREADS)
sse_fwd_kernel(const T* __restrict__ raw, const float* __restrict__ mean, const float* __restrict__ rstd, int C, SseParams p,
               T* __restrict__ e_out, SseHead head, long long V) {
  SEUNET_EPI_THREAD(LPV);
  float mu[8], rs[8], wse[8], wse2[8], w20[8], w21[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = mean[n * C + c0 + j];
    rs[j] = rstd[n * C + c0 + j];
    wse[j] = p.w_se[c0 + j];
    wse2[j] = G2 ? p.w_se2[c0 + j] : 0.f;
    w20[j] = p.w_side[c0 + j];
    w21[j] = p.w_side[C + c0 + j];
  }
  const float b20 = p.b_side[0], b21 = p.b_side[1], slope = p.slope;
  const bool want_side = head.side_out != nullptr || head.level_map != nullptr;
  float hw0 = 0.f, hw1 = 0.f;
  if (head.level_map) {
    hw0 = head.head_w[0] * (head.drop ? head.drop[n * head.drop_stride + 0] : 1.f);
    hw1 = head.head_w[1] * (head.drop ? head.drop[n * head.drop_stride + 1] : 1.f);
  }
  const long long stride = (long long)P * VPB;
  long long v = (long long)blockIdx.x * VPB + vb;
  Pack8<T> nx;   // software pipeline: voxel v + stride is loaded before voxel v is computed
  zero8p(nx);
  if (v < V) load8p(raw + ((long long)n * V + v) * C + c0, nx);
  for (; v < V; v += stride) {
    const long long vi = (long long)n * V + v;
    float x[8], a[8], e[8];
    unpack8(nx, x);
    if (v + stride < V) load8p(raw + (vi + stride) * C + c0, nx);
    float d1 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = norm_lrelu(x[j], mu[j], rs[j], slope);
      d1 += wse[j] * a[j];
    }
    const float g1 = gate_sigmoid<T>(group_sum<LPV>(d1));
    float d2 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      e[j] = a[j] * g1;
      d2 += wse2[j] * e[j];
    }
    if (G2) {
      const float g2 = gate_sigmoid<T>(group_sum<LPV>(d2));
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] *= g2;
    }
    store8(e_out + vi * C + c0, e);
    if (want_side) {     // (block-uniform; off for the encoder blocks of an inference forward that discards the encoder head)
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) { s0 += w20[j] * e[j]; s1 += w21[j] * e[j]; }
      s0 = group_sum<LPV>(s0) + b20;
      s1 = group_sum<LPV>(s1) + b21;
      if (cg == 0) {
        if (head.side_out) { head.side_out[vi * 2] = s0; head.side_out[vi * 2 + 1] = s1; }
        if (head.level_map) {
          const float t = hw0 * s0 + hw1 * s1;
          head.level_map[vi] = head.level_accumulate ? head.level_map[vi] + t : t;
        }
      }
    }
  }
}

// ----------------------------------------------------------------------------------
// gated block, backward.  The gradient w.r.t. the normalised activation (dxhat) is recomputed from the
// saved raw conv output in both passes and never stored:
//   APPLY = false (pass A): per-(n,c) sums of dxhat and dxhat*xhat (f64: the loss gradient has a large
//                           common-mode part that InstanceNorm's backward cancels, so f32 sums are not
//                           enough) + the gate / side / head parameter gradients
//   APPLY = true  (pass B): draw = rstd * (dxhat - m1 - xhat * m2), rounded once, stored over g_e
// ----------------------------------------------------------------------------------
// LEVEL: the side gradient arrives as ONE value per voxel, the gradient g of the head's level map (training: always), so
//   d side_k = hw_k * g with hw_k = head weight x DropLayer scale of the sample.  Everything that is linear in it is then taken out
//   of the voxel loop: de += g * (w20 hw0 + w21 hw1) with the bracket formed once per thread, and the gradients of the side conv,
//   its bias and the head weights all follow from G[c] = sum_v g e[c] and sum_v g at the end of the block (d w2k[c] = hw_k G[c],
//   d b2k = hw_k sum g, d head_k = drop_k (sum_c w2k[c] G[c] + b2k sum g)) -- no per-voxel side values, no second accumulator set.
//   Pass A of the one-gate C = 32 block: 266 -> ~200 instructions per voxel group, under its HBM time.
template <typename T, int LPV, bool G2, bool APPLY, bool LEVEL>
__global__ void __launch_bounds__(EPI_THREADS, (APPLY || G2) ? 1 : 3)
sse_bwd_kernel(const T* __restrict__ raw, const float* __restrict__ mean, const float* __restrict__ rstd, int C, SseParams p,
               SseBwdIn g, SseHead head, const float* __restrict__ m1p, const float* __restrict__ m2p, T* dxhat_out,
               double* __restrict__ stat_partial, float* __restrict__ pgrad_partial, long long V) {
  SEUNET_EPI_THREAD(LPV);
  float mu[8], rs[8], wse[8], wse2[8], w20[8], w21[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = mean[n * C + c0 + j];
    rs[j] = rstd[n * C + c0 + j];
    wse[j] = p.w_se[c0 + j];
    wse2[j] = G2 ? p.w_se2[c0 + j] : 0.f;
    w20[j] = p.w_side[c0 + j];
    w21[j] = p.w_side[C + c0 + j];
  }
  const float b20 = p.b_side[0], b21 = p.b_side[1], slope = p.slope;
  float dr0 = 1.f, dr1 = 1.f, hw0 = 0.f, hw1 = 0.f;
  if (g.g_level) {
    if (head.drop) { dr0 = head.drop[n * head.drop_stride]; dr1 = head.drop[n * head.drop_stride + 1]; }
    hw0 = head.head_w[0] * dr0;
    hw1 = head.head_w[1] * dr1;
  }
  // f64 sums live in thread-private LDS slots (pass A only): 32 fewer VGPRs than register accumulators, which is
  // the difference between 2 and 3 waves per SIMD for this latency-bound loop
  // bf16 activations: the thread's <= ~130 voxels are summed in f32 registers and converted once (the tensors keep 8
  // mantissa bits; gate = the bf16-autocast comparison), which frees the 32 KB of LDS slots -> twice the blocks per CU
  constexpr bool F64ACC = !APPLY && sizeof(T) == 4;   // (bf16 / f16 storage: f32 thread sums)
  __shared__ double acc64[F64ACC ? 16 : 1][F64ACC ? EPI_THREADS : 1];
  float fdx[8], fdxx[8];   // f32 staging of the f64 sums, flushed every 8 voxels
  float awse[8], awse2[8], aw20[8], aw21[8], am1[8], am2[8];
  int since_flush = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (F64ACC) acc64[j][threadIdx.x] = acc64[8 + j][threadIdx.x] = 0.0;
    fdx[j] = fdxx[j] = 0.f;
    awse[j] = awse2[j] = aw20[j] = aw21[j] = 0.f;
    am1[j] = APPLY ? m1p[n * C + c0 + j] : 0.f;
    am2[j] = APPLY ? m2p[n * C + c0 + j] : 0.f;
  }
  float adb0 = 0.f, adb1 = 0.f, adh0 = 0.f, adh1 = 0.f;
  float wc[8], sgl = 0.f;      // LEVEL: w20 hw0 + w21 hw1; sum of g (aw20 doubles as G)
#pragma unroll
  for (int j = 0; j < 8; ++j) wc[j] = w20[j] * hw0 + w21[j] * hw1;

  // software pipeline: the loads of voxel v + stride are issued before voxel v is computed
  const long long stride = (long long)P * VPB;
  long long v = (long long)blockIdx.x * VPB + vb;
  Pack8<T> nx, nde;
  float ngl = 0.f, ns0 = 0.f, ns1 = 0.f;
  zero8p(nx); zero8p(nde);
#define SSE_BWD_FETCH(vv)                                                                  \
  do {                                                                                     \
    const long long fi_ = (long long)n * V + (vv);                                         \
    load8p(raw + fi_ * C + c0, nx);                                                        \
    if (g.g_e) load8p(reinterpret_cast<const T*>(g.g_e) + fi_ * C + c0, nde);              \
    if (g.g_level) ngl = g.g_level[fi_];                                                   \
    else if (g.g_side) { ns0 = g.g_side[fi_ * 2]; ns1 = g.g_side[fi_ * 2 + 1]; }           \
  } while (0)
  if (v < V) SSE_BWD_FETCH(v);
  for (; v < V; v += stride) {
    const long long vi = (long long)n * V + v;
    float x[8], xh[8], a[8], b[8], e[8], de[8];
    unpack8(nx, x);
    unpack8(nde, de);
    const float gl = ngl, gs0 = ns0, gs1 = ns1;
    if (v + stride < V) SSE_BWD_FETCH(v + stride);
    float d1 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xh[j] = (x[j] - mu[j]) * rs[j];
      a[j] = lrelu(xh[j], slope);
      d1 += wse[j] * a[j];
    }
    const float g1 = gate_sigmoid<T>(group_sum<LPV>(d1));
    float d2 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { b[j] = a[j] * g1; d2 += wse2[j] * b[j]; }
    float g2 = 1.f;
    if (G2) g2 = gate_sigmoid<T>(group_sum<LPV>(d2));
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = G2 ? b[j] * g2 : b[j];

    // gradient arriving through the 2-channel side output
    float t2 = 0.f;
    if (LEVEL) {
      if (!APPLY) sgl += gl;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        de[j] += gl * wc[j];
        if (!APPLY) aw20[j] += gl * e[j];
        t2 += de[j] * b[j];
      }
    } else {
      float ds0 = 0.f, ds1 = 0.f;
      if (g.g_level) {
        ds0 = hw0 * gl;
        ds1 = hw1 * gl;
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { s0 += w20[j] * e[j]; s1 += w21[j] * e[j]; }
        s0 = group_sum<LPV>(s0) + b20;
        s1 = group_sum<LPV>(s1) + b21;
        if (!APPLY && cg == 0) { adh0 += gl * dr0 * s0; adh1 += gl * dr1 * s1; }
      } else if (g.g_side) {
        ds0 = gs0;
        ds1 = gs1;
      }
      if (cg == 0) { adb0 += ds0; adb1 += ds1; }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        de[j] += w20[j] * ds0 + w21[j] * ds1;
        aw20[j] += ds0 * e[j];
        aw21[j] += ds1 * e[j];
        t2 += de[j] * b[j];
      }
    }
    if (G2) {  // e = b * g2, g2 = sigmoid(<w_se2, b>)
      const float q2 = group_sum<LPV>(t2) * g2 * (1.f - g2);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        awse2[j] += q2 * b[j];
        de[j] = de[j] * g2 + q2 * wse2[j];  // now d/db
      }
    }
    float t1 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) t1 += de[j] * a[j];
    const float q1 = group_sum<LPV>(t1) * g1 * (1.f - g1);  // b = a * g1, g1 = sigmoid(<w_se, a>)
    float dxh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      awse[j] += q1 * a[j];
      const float da = de[j] * g1 + q1 * wse[j];
      dxh[j] = da * lrelu_slope(xh[j], slope);
      if (APPLY) {
        dxh[j] = rs[j] * (dxh[j] - am1[j] - xh[j] * am2[j]);
      } else {
        fdx[j] += dxh[j];
        fdxx[j] += dxh[j] * xh[j];
      }
    }
    if (APPLY) store8(dxhat_out + vi * C + c0, dxh);
    else if (F64ACC && ++since_flush == 8) {
      since_flush = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        acc64[j][threadIdx.x] += (double)fdx[j];
        acc64[8 + j][threadIdx.x] += (double)fdxx[j];
        fdx[j] = fdxx[j] = 0.f;
      }
    }
  }
#undef SSE_BWD_FETCH
  if (APPLY) return;
  if (LEVEL) {     // aw20 holds G[c] = sum_v g e[c]: the side / bias / head gradients of this thread's voxels follow from it
    float h0 = cg == 0 ? b20 * sgl : 0.f, h1 = cg == 0 ? b21 * sgl : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float G = aw20[j];
      h0 += w20[j] * G;
      h1 += w21[j] * G;
      aw20[j] = hw0 * G;
      aw21[j] = hw1 * G;
    }
    adh0 = dr0 * h0;
    adh1 = dr1 * h1;
    adb0 = cg == 0 ? hw0 * sgl : 0.f;
    adb1 = cg == 0 ? hw1 * sgl : 0.f;
  }
  double sdx[8], sdxx[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sdx[j] = (F64ACC ? acc64[j][threadIdx.x] : 0.0) + (double)fdx[j];
    sdxx[j] = (F64ACC ? acc64[8 + j][threadIdx.x] : 0.0) + (double)fdxx[j];
  }

  // ---- block reduction (fixed order) ----
  __shared__ double redd[4][16][16];
  __shared__ float red[4][16][32];
  __shared__ float reds[4][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const double r0 = stride_sum_d<LPV>(sdx[j]), r1 = stride_sum_d<LPV>(sdxx[j]);
    const float r2 = stride_sum<LPV>(awse[j]), r3 = stride_sum<LPV>(awse2[j]);
    const float r4 = stride_sum<LPV>(aw20[j]), r5 = stride_sum<LPV>(aw21[j]);
    if (lane < LPV) {
      redd[wave][lane][j] = r0;     redd[wave][lane][8 + j] = r1;
      red[wave][lane][j] = r2;      red[wave][lane][8 + j] = r3;
      red[wave][lane][16 + j] = r4; red[wave][lane][24 + j] = r5;
    }
  }
  {
    const float q0 = stride_sum<1>(adb0), q1 = stride_sum<1>(adb1);
    const float q2 = stride_sum<1>(adh0), q3 = stride_sum<1>(adh1);
    if (lane == 0) { reds[wave][0] = q0; reds[wave][1] = q1; reds[wave][2] = q2; reds[wave][3] = q3; }
  }
  __syncthreads();
  const long long rec = (long long)n * P + blockIdx.x;
  float* pg = pgrad_partial + rec * (4 * C + 4);
  for (int i = threadIdx.x; i < LPV * 16; i += EPI_THREADS) {
    const int gq = i / 16, k = i % 16;
    const double tot = wave4_sum(redd, gq, k);
    stat_partial[(rec * C + gq * 8 + (k & 7)) * 2 + (k >> 3)] = tot;
  }
  for (int i = threadIdx.x; i < LPV * 32; i += EPI_THREADS) {
    const int gq = i / 32, k = i % 32;
    const float tot = wave4_sum(red, gq, k);
    pg[(k >> 3) * C + gq * 8 + (k & 7)] = tot;
  }
  if (const int k = threadIdx.x; k < 4) pg[4 * C + k] = wave4_sum(reds, k);
}

// sums the per-block parameter-gradient records; one wave per entry, f64, fixed order
__device__ __forceinline__ void pgrad_reduce_body(int blk, const float* __restrict__ pg, int records, int C, float* dw_se,
                                                  float* dw_se2, float* dw_side, float* db_side, float* dhead_w) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = blk * 4 + wave, K = 4 * C + 4;
  if (k >= K) return;
  double s = 0.0;
  for (int r = lane; r < records; r += 64) s += (double)pg[(long long)r * K + k];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += shfl_xor_settled(s, off);
  if (lane != 0) return;
  const float v = (float)s;
  if (k < C) { if (dw_se) dw_se[k] = v; }
  else if (k < 2 * C) { if (dw_se2) dw_se2[k - C] = v; }
  else if (k < 4 * C) { if (dw_side) dw_side[k - 2 * C] = v; }
  else if (k < 4 * C + 2) { if (db_side) db_side[k - 4 * C] = v; }
  else { if (dhead_w) dhead_w[k - 4 * C - 2] = v; }
}
__global__ void __launch_bounds__(256)
pgrad_reduce_kernel(const float* __restrict__ pg, int records, int C, float* dw_se, float* dw_se2,
                    float* dw_side, float* db_side, float* dhead_w) {
  pgrad_reduce_body(blockIdx.x, pg, records, C, dw_se, dw_se2, dw_side, db_side, dhead_w);
}
// what follows pass A of a gated block, in ONE launch: the two means of the InstanceNorm backward (blocks [0, N*C)) and the
// parameter-gradient records (the next cdiv(4 * C + 4, 4) blocks) -- two dependent 5-us launches on the critical path otherwise.
// Any blocks past those are riders: the slab reduction of the weight gradient that ran before this block's pass A (wgrad.h),
// which nothing in this launch depends on and which depends on nothing in it.  The statistics blocks, which pass B waits
// for, come first in the grid and so dispatch first.
__global__ void __launch_bounds__(256)
gate_bwd_finalize_kernel(const double* __restrict__ partial, int slots, int C, int N, double inv_count, float* __restrict__ m1,
                         float* __restrict__ m2, const float* __restrict__ pg, int records, float* dw_se, float* dw_se2,
                         float* dw_side, float* db_side, float* dhead_w, WgReduceJob rider) {
  const int own = N * C + (4 * C + 4 + 3) / 4;   // (the launcher's grid without riders)
  if ((int)blockIdx.x < N * C) stats_finalize_body(blockIdx.x, partial, slots, C, inv_count, 0.f, 1, m1, m2);
  else if ((int)blockIdx.x < own) pgrad_reduce_body((int)blockIdx.x - N * C, pg, records, C, dw_se, dw_se2, dw_side, db_side, dhead_w);
  else wgrad_reduce_body(rider, (int)blockIdx.x - own);
}

int launch_sse_fwd(int dtype, const GateBlock& b, void* e_out, const SseHead& head, Dims d, hipStream_t s) {
  if (int e = check_c(b.C)) return e;
  dim3 grid(epi_partials(d) * 4, d.N);   // nothing is reduced here: enough blocks for full occupancy
  const bool g2 = b.p.w_se2 != nullptr;
  SEUNET_LPV_SWITCH(b.C / 8, {
    SEUNET_DTYPE_SWITCH(dtype, {
      if (g2) sse_fwd_kernel<T, LPV, true><<<grid, EPI_THREADS, 0, s>>>((const T*)b.a.raw, b.a.mean, b.a.rstd, b.C, b.p, (T*)e_out, head, d.vox());
      else sse_fwd_kernel<T, LPV, false><<<grid, EPI_THREADS, 0, s>>>((const T*)b.a.raw, b.a.mean, b.a.rstd, b.C, b.p, (T*)e_out, head, d.vox());
    });
  });
  SEUNET_LAUNCH_CHECK();
  return 0;
}

template <typename T, bool APPLY>
static int sse_bwd_t(const GateBlock& b, const SseBwdIn& g, const SseHead& head, const SseSums& o, const SseApply& a, Dims d,
                     hipStream_t s) {
  dim3 grid(epi_partials(d) * (APPLY ? 4 : 1), d.N);
  const bool g2 = b.p.w_se2 != nullptr;
  const bool level = g.g_level != nullptr;
#define SEUNET_SSE_BWD(G2V, LV) sse_bwd_kernel<T, LPV, G2V, APPLY, LV><<<grid, EPI_THREADS, 0, s>>>((const T*)b.a.raw, b.a.mean, b.a.rstd, b.C, b.p, g, head, a.m1, a.m2, (T*)a.draw_out, o.stat_partial, o.pgrad_partial, d.vox())
  SEUNET_LPV_SWITCH(b.C / 8, {
    if (g2) { if (level) SEUNET_SSE_BWD(true, true); else SEUNET_SSE_BWD(true, false); }
    else { if (level) SEUNET_SSE_BWD(false, true); else SEUNET_SSE_BWD(false, false); }
  });
#undef SEUNET_SSE_BWD
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_sse_bwd_sums(int dtype, const GateBlock& b, const SseBwdIn& g, const SseHead& head, const SseSums& out, Dims d,
                        hipStream_t s) {
  if (int e = check_c(b.C)) return e;
  SEUNET_CHECK(out.stat_partial && out.pgrad_partial, "gate_epilogue_bwd_sums needs the partial buffers");
  SEUNET_DTYPE_SWITCH(dtype, return (sse_bwd_t<T, false>(b, g, head, out, SseApply{}, d, s)));
  return 1;
}

int launch_sse_bwd_apply(int dtype, const GateBlock& b, const SseBwdIn& g, const SseHead& head, const SseApply& io, Dims d,
                         hipStream_t s) {
  if (int e = check_c(b.C)) return e;
  SEUNET_CHECK(io.m1 && io.m2 && io.draw_out, "gate_epilogue_bwd_apply needs m1, m2 and the output tensor");
  SEUNET_DTYPE_SWITCH(dtype, return (sse_bwd_t<T, true>(b, g, head, SseSums{}, io, d, s)));
  return 1;
}

int launch_gate_bwd_finalize(const double* stat_partial, int slots, int C, int N, long long count, float* m1, float* m2,
                             const float* pgrad_partial, int records, float* dw_se, float* dw_se2, float* dw_side,
                             float* db_side, float* dhead_w, hipStream_t s, const WgReduceJob* rider) {
  const WgReduceJob job = rider ? *rider : WgReduceJob{};
  gate_bwd_finalize_kernel<<<N * C + cdiv(4 * C + 4, 4) + job.blocks(), 256, 0, s>>>(
      stat_partial, slots, C, N, 1.0 / (double)count, m1, m2, pgrad_partial, records, dw_se, dw_se2, dw_side, db_side, dhead_w, job);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_pgrad_reduce(const float* pgrad_partial, int records, int C, float* dw_se, float* dw_se2, float* dw_side, float* db_side,
                        float* dhead_w, hipStream_t s) {
  pgrad_reduce_kernel<<<cdiv(4 * C + 4, 4), 256, 0, s>>>(pgrad_partial, records, C, dw_se, dw_se2, dw_side, db_side, dhead_w);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
