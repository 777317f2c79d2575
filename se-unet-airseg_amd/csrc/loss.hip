// Dice / General-Union / ATR losses (reference train.py:51-76), forward sums and backward, gfx950.
//
// All three losses are ratios of whole-batch sums, so one streaming pass produces the
// seven sums every loss needs and one streaming pass produces d(loss)/d(pred).  With
// apply_sigmoid=1 the kernels take raw logits (train.py:595-596 applies torch.sigmoid first) and the
// backward pass folds in sigmoid'.
//   sums[0] = sum p*t        sums[1] = sum p          sums[2] = sum t            (dice)
//   sums[3] = sum w*(p+1e-4)^0.7*t   sums[4] = sum w*(0.2 p + 0.8 t)              (general union)
//   sums[5] = sum w*(p*s)*s          sums[6] = sum w*(p*s + s)                    (ATR; s = skeleton)
#include "seunet_common.h"

namespace seunet {

static constexpr int LOSS_BLOCKS = 1024;   // 4 per CU; each thread handles n / (1024 * 256) elements, 4 per load
int loss_partials() { return LOSS_BLOCKS; }

// TERMS: bit 0 dice (sums 0-2), bit 1 general union (3-4), bit 2 ATR (5-6); sums of terms that are not asked for stay 0.
// (The pow of the general-union term costs more than everything else together, and a wave pays it as soon as ONE of its 256
// voxels is foreground: a Dice-only stage-1 step should not.)
template <int TERMS>
__device__ __forceinline__ void loss_terms(float p, int apply_sigmoid, float t, float w, float sk, float (&s)[SEUNET_LOSS_NSUMS]) {
  if (apply_sigmoid) p = 1.f / (1.f + expf(-p));
  // Every multiply-add is an explicit fmaf.  Left to the compiler the contraction differed between the instantiations (<2>
  // formed 0.2 p + 0.8 t from a packed multiply and an addition, <6> and <7> from a multiply and an fma), and a sum depended in
  // its last bits on which OTHER sums were asked for.
  if (TERMS & 1) {
    s[0] = fmaf(p, t, s[0]);
    s[1] += p;
    s[2] += t;
  }
  if (TERMS & 2) {
    if (t != 0.f) s[3] = fmaf(w * powf(p + 1e-4f, 0.7f), t, s[3]);   // (the label is sparse: the pow is skipped where it is multiplied by 0)
    s[4] = fmaf(w, fmaf(0.2f, p, 0.8f * t), s[4]);
  }
  if (TERMS & 4) {
    const float ps = p * sk;
    s[5] = fmaf(w * ps, sk, s[5]);
    s[6] = fmaf(w, ps + sk, s[6]);
  }
}

template <int TERMS>
__global__ void __launch_bounds__(256)
loss_sums_kernel(const float* __restrict__ pred, int apply_sigmoid, const float* __restrict__ target,
                 const float* __restrict__ weight, const float* __restrict__ skel, long long n,
                 float* __restrict__ partial) {
  float s[SEUNET_LOSS_NSUMS];
#pragma unroll
  for (int k = 0; k < SEUNET_LOSS_NSUMS; ++k) s[k] = 0.f;
  const bool vec = (n & 3) == 0 && ((reinterpret_cast<size_t>(pred) | reinterpret_cast<size_t>(target) |
                                     reinterpret_cast<size_t>(weight) | reinterpret_cast<size_t>(skel)) & 15) == 0;
  if (vec) {   // 16-byte loads
    const long long n4 = n >> 2;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
      const float4 p = reinterpret_cast<const float4*>(pred)[i], t = reinterpret_cast<const float4*>(target)[i];
      const float4 w = weight ? reinterpret_cast<const float4*>(weight)[i] : make_float4(1.f, 1.f, 1.f, 1.f);
      const float4 k = skel ? reinterpret_cast<const float4*>(skel)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      loss_terms<TERMS>(p.x, apply_sigmoid, t.x, w.x, k.x, s);
      loss_terms<TERMS>(p.y, apply_sigmoid, t.y, w.y, k.y, s);
      loss_terms<TERMS>(p.z, apply_sigmoid, t.z, w.z, k.z, s);
      loss_terms<TERMS>(p.w, apply_sigmoid, t.w, w.w, k.w, s);
    }
  } else {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
      loss_terms<TERMS>(pred[i], apply_sigmoid, target[i], weight ? weight[i] : 1.f, skel ? skel[i] : 0.f, s);
  }
  __shared__ float red[4][SEUNET_LOSS_NSUMS];
#pragma unroll
  for (int k = 0; k < SEUNET_LOSS_NSUMS; ++k) {
    float v = s[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += shfl_xor_settled(v, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < SEUNET_LOSS_NSUMS) {
    const int k = threadIdx.x;
    partial[blockIdx.x * SEUNET_LOSS_NSUMS + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// one wave per sum: lane l adds the block partials l, l+64, ... in f64, then a fixed-order butterfly
__global__ void __launch_bounds__(64 * SEUNET_LOSS_NSUMS)
loss_sums_final_kernel(const float* __restrict__ partial, int blocks, double* __restrict__ sums) {
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double s = 0.0;
  for (int b = lane; b < blocks; b += 64) s += (double)partial[b * SEUNET_LOSS_NSUMS + k];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += shfl_xor_settled(s, off);
  if (lane == 0) sums[k] = s;
}

// g_pred[i] = g_scale * ( c_dice*d dice/dp + c_gul*d gul/dp + c_atr*d atr/dp ) [* p(1-p)]
__global__ void __launch_bounds__(256)
loss_grad_kernel(const float* __restrict__ pred, int apply_sigmoid, const float* __restrict__ target,
                 const float* __restrict__ weight, const float* __restrict__ skel, long long n,
                 const double* __restrict__ sums, float c_dice, float c_gul, float c_atr, float g_scale,
                 const float* __restrict__ g_scale_dev, float* __restrict__ g_pred) {
  if (g_scale_dev) g_scale *= g_scale_dev[0];
  // dice = 1 - (2I+1)/(P+T+1)
  const float dA = (float)(2.0 * sums[0] + 1.0), dB = (float)(sums[1] + sums[2] + 1.0);
  // gul = 1 - (A+1)/(B+1)
  const float gA = (float)(sums[3] + 1.0), gB = (float)(sums[4] + 1.0);
  // atr = 1 - (C1+1)/(C2+1)
  const float aA = (float)(sums[5] + 1.0), aB = (float)(sums[6] + 1.0);
  auto grad1 = [&](float p, float t, float w, float sk) -> float {
    if (apply_sigmoid) p = 1.f / (1.f + expf(-p));
    float g = 0.f;
    if (c_dice != 0.f) g += c_dice * (-(2.f * t * dB - dA) / (dB * dB));
    if (c_gul != 0.f) {
      const float dnum = (t != 0.f) ? 0.7f * w * t * powf(p + 1e-4f, -0.3f) : 0.f;
      g += c_gul * (-(dnum * gB - gA * 0.2f * w) / (gB * gB));
    }
    if (c_atr != 0.f) g += c_atr * (-(w * sk * sk * aB - aA * w * sk) / (aB * aB));
    g *= g_scale;
    if (apply_sigmoid) g *= p * (1.f - p);
    return g;
  };
  const bool vec = (n & 3) == 0 && ((reinterpret_cast<size_t>(pred) | reinterpret_cast<size_t>(target) | reinterpret_cast<size_t>(weight) |
                                     reinterpret_cast<size_t>(skel) | reinterpret_cast<size_t>(g_pred)) & 15) == 0;
  if (vec) {
    const long long n4 = n >> 2;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
      const float4 p = reinterpret_cast<const float4*>(pred)[i], t = reinterpret_cast<const float4*>(target)[i];
      const float4 w = weight ? reinterpret_cast<const float4*>(weight)[i] : make_float4(1.f, 1.f, 1.f, 1.f);
      const float4 k = skel ? reinterpret_cast<const float4*>(skel)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      reinterpret_cast<float4*>(g_pred)[i] = make_float4(grad1(p.x, t.x, w.x, k.x), grad1(p.y, t.y, w.y, k.y),
                                                         grad1(p.z, t.z, w.z, k.z), grad1(p.w, t.w, w.w, k.w));
    }
  } else {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
      g_pred[i] = grad1(pred[i], target[i], weight ? weight[i] : 1.f, skel ? skel[i] : 0.f);
  }
}

int launch_loss_sums(const float* pred, int apply_sigmoid, const float* target, const float* weight,
                     const float* skel, long long n, float* partial, double* sums, hipStream_t s, int terms) {
  terms &= 7;
  if (terms == 0) terms = 7;
  switch (terms) {
    case 1: loss_sums_kernel<1><<<LOSS_BLOCKS, 256, 0, s>>>(pred, apply_sigmoid, target, weight, skel, n, partial); break;
    case 2: loss_sums_kernel<2><<<LOSS_BLOCKS, 256, 0, s>>>(pred, apply_sigmoid, target, weight, skel, n, partial); break;
    case 6: loss_sums_kernel<6><<<LOSS_BLOCKS, 256, 0, s>>>(pred, apply_sigmoid, target, weight, skel, n, partial); break;
    default: loss_sums_kernel<7><<<LOSS_BLOCKS, 256, 0, s>>>(pred, apply_sigmoid, target, weight, skel, n, partial); break;
  }
  loss_sums_final_kernel<<<1, 64 * SEUNET_LOSS_NSUMS, 0, s>>>(partial, LOSS_BLOCKS, sums);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// loss value from the (already all-reduced) sums of one or two heads, formed on the device in f64 and rounded to f32 per
// head like the reference's scalar arithmetic (train.py:51-76 on whole-batch sums): value = f32(head 0) + f32(head 1)
__global__ void loss_value_kernel(const double* __restrict__ s0, double d0, double g0, double a0,
                                  const double* __restrict__ s1, double d1, double g1, double a1, float* __restrict__ value) {
  auto one = [](const double* s, double cd, double cg, double ca) -> float {
    double out = 0.0;
    if (cd != 0.0) out = out + cd * (1.0 - (2.0 * s[0] + 1.0) / (s[1] + s[2] + 1.0));
    if (cg != 0.0) out = out + cg * (1.0 - (s[3] + 1.0) / (s[4] + 1.0));
    if (ca != 0.0) out = out + ca * (1.0 - (s[5] + 1.0) / (s[6] + 1.0));
    return (float)out;
  };
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float v = one(s0, d0, g0, a0);
    if (s1 != nullptr) v = v + one(s1, d1, g1, a1);
    value[0] = v;
  }
}

int launch_loss_value(const double* sums0, double c_dice0, double c_gul0, double c_atr0, const double* sums1, double c_dice1,
                      double c_gul1, double c_atr1, float* value, hipStream_t s) {
  loss_value_kernel<<<1, 64, 0, s>>>(sums0, c_dice0, c_gul0, c_atr0, sums1, c_dice1, c_gul1, c_atr1, value);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// ---- per-sample sums and values: the online-hard-mining key (train.py:442-446, :249-253) -------------------------------------
// The reference re-evaluates general_union_loss_lib(pred_de[i], label[i], weight[i]) once per sample with a .item() each.  Here
// one pass gives the seven sums of every sample: grid (SAMPLE_BLOCKS, batch), block (x, b) strides over sample b's elements
// [b n, (b + 1) n) exactly as loss_sums_kernel strides over the whole array, and reduces with the same tree.  Nothing in a
// block's work depends on gridDim.y or on another sample, so sample b's sums are the same bits alone or in any batch.
// (The body restates loss_sums_kernel's instead of sharing a function with it: that kernel's code object stays as it is.)
static constexpr int SAMPLE_BLOCKS = 256;                    // per sample: 1 per CU; 8 trips of the 16-byte path at 128^3
static constexpr int SAMPLE_STRIDE = SAMPLE_BLOCKS * 256;    // threads that share one sample
int loss_sample_partials(int batch) { return batch * SAMPLE_BLOCKS; }

template <int TERMS>
__global__ void __launch_bounds__(256)
loss_sample_sums_kernel(const float* __restrict__ pred, int apply_sigmoid, const float* __restrict__ target,
                        const float* __restrict__ weight, const float* __restrict__ skel, long long n,
                        float* __restrict__ partial) {
  const long long base = (long long)blockIdx.y * n;
  pred += base;
  target += base;
  if (weight) weight += base;
  if (skel) skel += base;
  float s[SEUNET_LOSS_NSUMS];
#pragma unroll
  for (int k = 0; k < SEUNET_LOSS_NSUMS; ++k) s[k] = 0.f;
  const bool vec = (n & 3) == 0 && ((reinterpret_cast<size_t>(pred) | reinterpret_cast<size_t>(target) |
                                     reinterpret_cast<size_t>(weight) | reinterpret_cast<size_t>(skel)) & 15) == 0;
  if (vec) {   // 16-byte loads
    const long long n4 = n >> 2;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += SAMPLE_STRIDE) {
      const float4 p = reinterpret_cast<const float4*>(pred)[i], t = reinterpret_cast<const float4*>(target)[i];
      const float4 w = weight ? reinterpret_cast<const float4*>(weight)[i] : make_float4(1.f, 1.f, 1.f, 1.f);
      const float4 k = skel ? reinterpret_cast<const float4*>(skel)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      loss_terms<TERMS>(p.x, apply_sigmoid, t.x, w.x, k.x, s);
      loss_terms<TERMS>(p.y, apply_sigmoid, t.y, w.y, k.y, s);
      loss_terms<TERMS>(p.z, apply_sigmoid, t.z, w.z, k.z, s);
      loss_terms<TERMS>(p.w, apply_sigmoid, t.w, w.w, k.w, s);
    }
  } else {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += SAMPLE_STRIDE)
      loss_terms<TERMS>(pred[i], apply_sigmoid, target[i], weight ? weight[i] : 1.f, skel ? skel[i] : 0.f, s);
  }
  __shared__ float red[4][SEUNET_LOSS_NSUMS];
#pragma unroll
  for (int k = 0; k < SEUNET_LOSS_NSUMS; ++k) {
    float v = s[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += shfl_xor_settled(v, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < SEUNET_LOSS_NSUMS) {
    const int k = threadIdx.x;
    partial[((long long)blockIdx.y * SAMPLE_BLOCKS + blockIdx.x) * SEUNET_LOSS_NSUMS + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// block b: sample b; one wave per sum, lane l adds that sample's block partials l, l+64, ... in f64, then the fixed-order butterfly
__global__ void __launch_bounds__(64 * SEUNET_LOSS_NSUMS)
loss_sample_final_kernel(const float* __restrict__ partial, double* __restrict__ sums) {
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  partial += (long long)blockIdx.x * SAMPLE_BLOCKS * SEUNET_LOSS_NSUMS;
  double s = 0.0;
  for (int b = lane; b < SAMPLE_BLOCKS; b += 64) s += (double)partial[b * SEUNET_LOSS_NSUMS + k];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += shfl_xor_settled(s, off);
  if (lane == 0) sums[(long long)blockIdx.x * SEUNET_LOSS_NSUMS + k] = s;
}

int launch_loss_sums_per_sample(const float* pred, int apply_sigmoid, const float* target, const float* weight, const float* skel,
                                int batch, long long n, float* partial, double* sums, int terms, hipStream_t s) {
  terms &= 7;
  if (terms == 0) terms = 7;
  const dim3 grid(SAMPLE_BLOCKS, batch);
  switch (terms) {
    case 1: loss_sample_sums_kernel<1><<<grid, 256, 0, s>>>(pred, apply_sigmoid, target, weight, skel, n, partial); break;
    case 2: loss_sample_sums_kernel<2><<<grid, 256, 0, s>>>(pred, apply_sigmoid, target, weight, skel, n, partial); break;
    case 6: loss_sample_sums_kernel<6><<<grid, 256, 0, s>>>(pred, apply_sigmoid, target, weight, skel, n, partial); break;
    default: loss_sample_sums_kernel<7><<<grid, 256, 0, s>>>(pred, apply_sigmoid, target, weight, skel, n, partial); break;
  }
  loss_sample_final_kernel<<<batch, 64 * SEUNET_LOSS_NSUMS, 0, s>>>(partial, sums);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// values[b]: the f64 ratio arithmetic of loss_value_kernel on sample b's sums, rounded once to f32
__global__ void __launch_bounds__(64)
loss_sample_values_kernel(const double* __restrict__ sums, int batch, double cd, double cg, double ca, float* __restrict__ values) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= batch) return;
  const double* s = sums + (long long)b * SEUNET_LOSS_NSUMS;
  double out = 0.0;
  if (cd != 0.0) out = out + cd * (1.0 - (2.0 * s[0] + 1.0) / (s[1] + s[2] + 1.0));
  if (cg != 0.0) out = out + cg * (1.0 - (s[3] + 1.0) / (s[4] + 1.0));
  if (ca != 0.0) out = out + ca * (1.0 - (s[5] + 1.0) / (s[6] + 1.0));
  values[b] = (float)out;
}

int launch_loss_sample_values(const double* sums, int batch, double c_dice, double c_gul, double c_atr, float* values, hipStream_t s) {
  loss_sample_values_kernel<<<(batch + 63) / 64, 64, 0, s>>>(sums, batch, c_dice, c_gul, c_atr, values);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_loss_grad(const float* pred, int apply_sigmoid, const float* target, const float* weight,
                     const float* skel, long long n, const double* sums, float c_dice, float c_gul,
                     float c_atr, float g_scale, const float* g_scale_dev, float* g_pred, hipStream_t s) {
  long long g = (n + 255) / 256;
  if (g > 4096) g = 4096;
  loss_grad_kernel<<<(int)g, 256, 0, s>>>(pred, apply_sigmoid, target, weight, skel, n, sums, c_dice, c_gul,
                                           c_atr, g_scale, g_scale_dev, g_pred);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
