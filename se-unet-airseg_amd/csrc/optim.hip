// Fused multi-tensor AdamW step.  Reference: the training loops call
// torch.optim.AdamW(model.parameters(), lr=0.0001) with default betas / eps / weight_decay (train.py:188,386,569) and
// optimizer.step() once per iteration (train.py:245-247,437-439,601-603): 117 small tensors, which eager PyTorch
// updates with ~18 multi-tensor launches.  Here every tensor of a step is updated by a handful of launches (up to
// 24 tensors per launch, their pointers travel in the kernel arguments: no device-side table, no workspace).
//
// Per element, decoupled weight decay and bias-corrected moments (torch/optim/adamw.py, _single_tensor_adamw; the
// reference pins pytorch 2.0.1, environment.yml:78):
//     p  <- p * (1 - lr * wd)
//     m  <- b1 * m + (1 - b1) * g
//     v  <- b2 * v + (1 - b2) * g * g
//     p  <- p - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// HBM-bound: 16 B read + 12 B written per parameter (6 MB of parameters: microseconds); f32 arithmetic.
//
// Gated form (launch_adamw_gated): a step behind a backward pass whose scaled fp16 gradients overflowed must change nothing.
// The decision is a device flag (int, non-zero = skip) that the backward pass wrote earlier on the stream; no host read.  Per
// launch a one-block prepare kernel reads the flag; on a skip it adds one to each tensor's device count of skipped steps,
// otherwise it forms step_size and 1/sqrt(bc2) in f64 from the tensor's effective step (host step - skipped) and writes them
// into a two-floats-per-tensor table.  The main kernel returns at once when the flag is set and reads the two scalars from
// the table otherwise; its arithmetic is the ungated kernel's.  The caller clears the flag after the last launch of a step.
#include "seunet_common.h"

namespace seunet {

constexpr int AW_MAX = 24;      // tensors per launch
constexpr int AW_CHUNK = 1024;  // elements per block
struct AdamwArgs {
  float* p[AW_MAX];
  const float* g[AW_MAX];
  float* m[AW_MAX];
  float* v[AW_MAX];
  long long count[AW_MAX];
  int first_block[AW_MAX + 1];   // prefix sums of ceil(count / AW_CHUNK)
  int n;
  float b1, b2, omb1, omb2, eps, decay, step_size, inv_sqrt_bc2, gsign;   // derived constants are formed in f64 on the host
};

struct AdamwGate {
  const int* flag;       // non-zero: the step is skipped
  const float* table;    // [2 * AW_MAX] of this launch: step_size, inv_sqrt_bc2 per tensor (written by adamw_prepare_kernel)
};
struct AdamwPrepareArgs {
  float* skipped[AW_MAX];   // per tensor: steps skipped so far (a whole number in an f32, the type optimizer state travels in)
  int step[AW_MAX];         // per tensor: state['step'] after the increment, skipped steps included
  int n;
  double lr, b1, b2;
};

__global__ void __launch_bounds__(64) adamw_prepare_kernel(AdamwPrepareArgs a, const int* __restrict__ flag, float* __restrict__ table) {
  const int i = threadIdx.x;
  if (i >= a.n) return;
  float sk = *a.skipped[i];
  if (*flag != 0) {
    *a.skipped[i] = sk + 1.f;
    return;                 // the main kernel does not read the table of a skipped step
  }
  int eff = a.step[i] - (int)sk;
  if (eff < 1) eff = 1;
  const double bc1 = 1.0 - pow(a.b1, (double)eff), bc2 = 1.0 - pow(a.b2, (double)eff);
  table[2 * i] = (float)(a.lr / bc1);
  table[2 * i + 1] = (float)(1.0 / sqrt(bc2));
}

template <bool GATED>
__global__ void __launch_bounds__(256) adamw_kernel(AdamwArgs a, AdamwGate gate) {
  if constexpr (GATED) {
    if (*gate.flag != 0) return;
  }
  // which tensor does this block belong to (n <= 24: linear scan on scalars)
  int t = 0;
  while (t + 1 < a.n && (int)blockIdx.x >= a.first_block[t + 1]) ++t;
  const long long base = (long long)((int)blockIdx.x - a.first_block[t]) * AW_CHUNK;
  float* __restrict__ p = a.p[t];
  const float* __restrict__ g = a.g[t];
  float* __restrict__ m = a.m[t];
  float* __restrict__ v = a.v[t];
  const long long cnt = a.count[t];
  const float decay = a.decay;
  float step_size = a.step_size, inv_sqrt_bc2 = a.inv_sqrt_bc2;
  if constexpr (GATED) {
    step_size = gate.table[2 * t];
    inv_sqrt_bc2 = gate.table[2 * t + 1];
  }
#pragma unroll
  for (int k = 0; k < AW_CHUNK / 256; ++k) {
    const long long i = base + k * 256 + threadIdx.x;
    if (i < cnt) {
      const float gi = a.gsign * g[i];
      const float pi = p[i] * decay;
      const float mi = a.b1 * m[i] + a.omb1 * gi;
      const float vi = a.b2 * v[i] + a.omb2 * gi * gi;
      const float denom = sqrtf(vi) * inv_sqrt_bc2 + a.eps;
      m[i] = mi;
      v[i] = vi;
      p[i] = pi - step_size * (mi / denom);
    }
  }
}

// fills the pointers, counts, block prefix sums and step-independent constants of tensors [base, base + a.n); returns the blocks,
// or -1 with the error set
static long long adamw_fill(AdamwArgs& a, float* const* params, const float* const* grads, float* const* exp_avg,
                            float* const* exp_avg_sq, const long long* counts, int base, double lr, double beta1, double beta2,
                            double eps, double weight_decay, int maximize) {
  long long blocks = 0;
  for (int i = 0; i < a.n; ++i) {
    if (!(params[base + i] && grads[base + i] && exp_avg[base + i] && exp_avg_sq[base + i] && counts[base + i] >= 0)) {
      fail("adamw: tensor %d has a null pointer or a negative size", base + i);
      return -1;
    }
    a.p[i] = params[base + i]; a.g[i] = grads[base + i]; a.m[i] = exp_avg[base + i]; a.v[i] = exp_avg_sq[base + i];
    a.count[i] = counts[base + i];
    a.first_block[i] = (int)blocks;
    blocks += (counts[base + i] + AW_CHUNK - 1) / AW_CHUNK;
    if (blocks >= (1LL << 31)) {
      fail("adamw: too many elements in one launch");
      return -1;
    }
  }
  a.first_block[a.n] = (int)blocks;
  a.b1 = (float)beta1; a.b2 = (float)beta2; a.eps = (float)eps;
  a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2);
  a.decay = (float)(1.0 - lr * weight_decay);
  a.gsign = maximize ? -1.f : 1.f;
  return blocks;
}

static int adamw_check_hyper(double lr, double beta1, double beta2, double eps, double weight_decay) {
  SEUNET_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && lr >= 0.0 && weight_decay >= 0.0,
               "adamw: invalid hyper-parameter");
  return 0;
}

int launch_adamw(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                 const long long* counts, int n, double lr, double beta1, double beta2, double eps, double weight_decay,
                 int step, int maximize, hipStream_t s) {
  SEUNET_CHECK(n >= 0 && step >= 1, "adamw: n=%d step=%d (step counts from 1)", n, step);
  if (adamw_check_hyper(lr, beta1, beta2, eps, weight_decay)) return 1;
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  for (int base = 0; base < n; base += AW_MAX) {
    AdamwArgs a{};
    a.n = n - base < AW_MAX ? n - base : AW_MAX;
    const long long blocks = adamw_fill(a, params, grads, exp_avg, exp_avg_sq, counts, base, lr, beta1, beta2, eps, weight_decay, maximize);
    if (blocks < 0) return 1;
    a.step_size = (float)(lr / bc1);
    a.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    if (blocks > 0) adamw_kernel<false><<<(unsigned)blocks, 256, 0, s>>>(a, AdamwGate{});
  }
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_adamw_gated(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                       const long long* counts, const int* steps, float* const* skipped, int n, double lr, double beta1,
                       double beta2, double eps, double weight_decay, int maximize, const int* flag, float* table, hipStream_t s) {
  SEUNET_CHECK(n >= 0 && flag && (n == 0 || (steps && skipped && table)), "adamw_gated: n=%d, or a null flag / steps / skipped / table", n);
  if (adamw_check_hyper(lr, beta1, beta2, eps, weight_decay)) return 1;
  for (int base = 0; base < n; base += AW_MAX) {
    AdamwArgs a{};
    AdamwPrepareArgs pa{};
    a.n = pa.n = n - base < AW_MAX ? n - base : AW_MAX;
    const long long blocks = adamw_fill(a, params, grads, exp_avg, exp_avg_sq, counts, base, lr, beta1, beta2, eps, weight_decay, maximize);
    if (blocks < 0) return 1;
    for (int i = 0; i < a.n; ++i) {
      SEUNET_CHECK(skipped[base + i] && steps[base + i] >= 1, "adamw_gated: tensor %d has no skipped-step count or step %d < 1",
                   base + i, steps[base + i]);
      pa.skipped[i] = skipped[base + i];
      pa.step[i] = steps[base + i];
    }
    pa.lr = lr; pa.b1 = beta1; pa.b2 = beta2;
    float* tab = table + 2 * base;
    // the prepare kernel also counts the skipped step of an empty tensor, so it runs even when there are no blocks
    adamw_prepare_kernel<<<1, 64, 0, s>>>(pa, flag, tab);
    if (blocks > 0) adamw_kernel<true><<<(unsigned)blocks, 256, 0, s>>>(a, AdamwGate{flag, tab});
  }
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
