// Shared layer of the block epilogues (epilogue.hip: channel statistics; gate.hip: the gated block; cat.hip: the aggregation
// block and its x-branch): their launcher prototypes and argument structs, and those device steps of their kernels that
// could be shared without changing the generated code.  Still spelled out per kernel: the mean / rstd and x-branch weight
// loads, the two-branch value and the per-channel block record (stride sums -> red[wave][lane][k] -> wave-order sum).
//
// Thread mapping of every pass: one lane owns 8 consecutive channels (16 B bf16 / 32 B f32) of one voxel, LPV = C/8 consecutive
// lanes own one voxel, so every global access is a fully coalesced 16/32-byte-per-lane stream, software-pipelined one voxel
// ahead; the per-voxel channel dot products of the gates are LPV-lane reductions on DPP (quad_perm / row_half_mirror /
// row_mirror), the per-(n,c) InstanceNorm sums are f64: strided shuffle reductions + a fixed-order cross-wave sum
// (deterministic, no atomics).
#pragma once
#include "seunet_common.h"

namespace seunet {

// ---- launchers and their arguments -----------------------------------------------------------------------------------
// A finalize launch between pass A and pass B can carry a rider: the slab reduction of an earlier weight gradient (wgrad.h,
// WgReduceJob) as extra workgroups after its own.  Null: none.
struct WgReduceJob;
int epi_partials(Dims d);         // partial slots per sample used by the epilogue kernels
int launch_channel_stats(int dtype, const void* t, int C, double* partial, Dims d, hipStream_t s);
int launch_stats_finalize(const double* partial, int slots, int C, int N, long long count,
                          float eps, int mode, float* out_a, float* out_b, hipStream_t s);
// A block's epilogue is described once and handed to its forward and to both backward passes.  The backward runs twice over
// the block: the `_sums` launchers (pass A) write f64 partial sums -- of the InstanceNorm backward's two means per (n, c),
// and of the parameter gradients -- and the `_apply` launchers (pass B) read the finalised means m1 / m2 and store draw.
// Each pass has its own argument struct, so that it cannot be handed the other pass's buffers.
struct NormIn { const void* raw; const float* mean; const float* rstd; };   // a conv output [N][V][C] (T), its InstanceNorm statistics [N][C]
struct SseParams {
  const float* w_se;      // [C]
  const float* w_se2;     // [C] or null (one gate)
  const float* w_side;    // [2][C]
  const float* b_side;    // [2]
  float slope;
};
struct GateBlock { NormIn a; int C; SseParams p; };
struct SseHead {          // how the 2-channel side output is consumed
  float* side_out;        // fp32 [N][V][2] or null
  float* level_map;       // fp32 [N][V] head pre-activation map of this level, or null
  int level_accumulate;   // 0: overwrite level_map, 1: +=
  const float* head_w;    // [2] head weights of this block's two channels
  const float* drop;      // [N][drop_stride] DropLayer scales (points at this block's channel 0) or null
  int drop_stride;
};
struct SseBwdIn {
  const void* g_e;        // gradient w.r.t. e (T) or null
  const float* g_side;    // fp32 [N][V][2] gradient w.r.t. the side map, or null
  const float* g_level;   // fp32 [N][V] gradient w.r.t. the level map, or null
};
// partial parameter-gradient record per (sample, slot):  4*C + 4 floats
//   [0,C) dw_se  [C,2C) dw_se2  [2C,4C) dw_side[2][C]  [4C,4C+2) db_side  [4C+2,4C+4) dhead_w
struct SseSums { double* stat_partial; float* pgrad_partial; };            // pass A outputs
struct SseApply { const float* m1; const float* m2; void* draw_out; };     // pass B; draw_out may alias g_e
int launch_sse_fwd(int dtype, const GateBlock& b, void* e_out, const SseHead& head, Dims d, hipStream_t s);
int launch_sse_bwd_sums(int dtype, const GateBlock& b, const SseBwdIn& g, const SseHead& head, const SseSums& out, Dims d,
                        hipStream_t s);
int launch_sse_bwd_apply(int dtype, const GateBlock& b, const SseBwdIn& g, const SseHead& head, const SseApply& io, Dims d,
                         hipStream_t s);
int launch_gate_bwd_finalize(const double* stat_partial, int slots, int C, int N, long long count, float* m1, float* m2,
                             const float* pgrad_partial, int records, float* dw_se, float* dw_se2, float* dw_side,
                             float* db_side, float* dhead_w, hipStream_t s, const WgReduceJob* rider = nullptr);
int launch_pgrad_reduce(const float* pgrad_partial, int records, int C, float* dw_se,
                        float* dw_se2, float* dw_side, float* db_side, float* dhead_w,
                        hipStream_t s);
struct Branch2 {          // the second branch of an aggregation block, added after its own InstanceNorm + LeakyReLU
  enum Kind { None, Stored, Recomputed } kind;
  const void* src;        // Stored: raw2 [N][V][C] (T); Recomputed: the packed network input [N][V][8] (T), raw2 = w2 x per voxel
  const float* mean2;
  const float* rstd2;
  const float* w2;        // Recomputed: the 1x1x1 weight (C, in_channel) and in_channel (1 or 2)
  int in_channel;
};
struct CatBlock { NormIn a; Branch2 b; int C; float slope; };
// Recomputed only.  Forward: also write the 2x2x2 max-pool of the output (pooled null = not) and, if asked, each maximum's position.
// Backward: the gradient of that max-pool, added to g_out on the fly in both passes (argmax null = none).
struct PoolOut { void* pooled; unsigned* argmax; };
struct PoolGrad { const unsigned* argmax; const void* g_pool; };
struct CatSums {          // pass A outputs
  double* stat_partial;
  double* stat_partial2;  // second branch (Stored | Recomputed)
  double* xw_partial;     // optional, Recomputed: one record per block of the x-branch weight-gradient sums (cat_bwd_kernel XW)
};
struct CatApply {         // pass B
  const float *m1, *m2, *m1b, *m2b;   // (m1b, m2b: second branch)
  void* dx;               // may alias g_out
  void* dx2;              // Stored: draw of the second branch
  float* gx_out;          // optional, Recomputed: + the x-branch's input-gradient term (XG), [N][V][in_channel] f32
  int gx_acc;             // 0: overwrite gx_out, 1: +=
};
int launch_cat_fwd(int dtype, const CatBlock& b, void* out, const PoolOut& pool, Dims d, hipStream_t s);
int launch_cat_bwd_sums(int dtype, const CatBlock& b, const void* g_out, const PoolGrad& pool, const CatSums& out, Dims d,
                        hipStream_t s);
int launch_cat_bwd_apply(int dtype, const CatBlock& b, const void* g_out, const PoolGrad& pool, const CatApply& io, Dims d,
                         hipStream_t s);
int xbranch_moment_slots(Dims d);
int launch_xbranch_moments(int dtype, const void* x_in, double* partial, Dims d, hipStream_t s);
int launch_xbranch_stats(const double* partial, int slots, const float* w2, int C, int in_channel, int N, long long count,
                         float eps, float* mean2, float* rstd2, double* moments_out, hipStream_t s);
int launch_cat_xgrad_finalize(const double* xw_partial, const double* stat_partial2, int slots, const double* moments, const float* w2,
                              int C, int in_channel, int N, float eps, float* dw, hipStream_t s);
// What follows pass A of an aggregation block, in ONE launch: the two means of the first branch (stat_partial -> m1, m2), those
// of the second (stat_partial2 -> m1b, m2b; null = one branch), the recomputed x-branch's weight gradient (xw.dw null = not
// asked for; what launch_cat_xgrad_finalize computes), then the rider.
struct CatXwFinalize { const double* xw_partial; const double* moments; const float* w2; int in_channel; float eps; float* dw; };
int launch_cat_bwd_finalize(const double* stat_partial, const double* stat_partial2, int slots, int C, int N, long long count,
                            float* m1, float* m2, float* m1b, float* m2b, const CatXwFinalize& xw, hipStream_t s,
                            const WgReduceJob* rider = nullptr);
int launch_xbranch_values(int dtype, const void* x_in, const float* w2, int C, int in_channel, float* out_ncdhw, Dims d, hipStream_t s);   // diagnostic

// ---- device steps ----------------------------------------------------------------------------------------------------
#ifdef __HIPCC__
static constexpr int EPI_THREADS = 256;

// the value a store of type T keeps (round to nearest even for the 16-bit types, the same conversion store8 uses)
template <typename T> __device__ __forceinline__ float round_to(float v) {
  if constexpr (sizeof(T) == 4) return v;
  else return unpack_lo<T>(pack2<T>(v, 0.f));
}

// The spatial gates' sigmoid.  f32 storage (the 1e-3 parity mode): expf and an IEEE division.  16-bit storage: one v_exp_f32 and
// one v_rcp_f32 (1 ulp each) instead of ~25 instructions of range reduction and division fix-up -- the gate multiplies values that
// keep 8 / 11 mantissa bits; forward and both backward passes use the same function, so a gate is the same number everywhere.
template <typename T> __device__ __forceinline__ float gate_sigmoid(float z) {
  if constexpr (sizeof(T) == 4) return 1.f / (1.f + expf(-z));
  else return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.44269504088896341f * z));
}

// The thread mapping of every voxel pass on a (partials, N) grid of EPI_THREADS-thread blocks: sample n, block record
// blockIdx.x of P, the 8-channel group cg of LPV (channels [c0, c0 + 8)), voxel slot vb of the block's VPB; the thread's
// voxels are blockIdx.x * VPB + vb, + P * VPB, ...  A macro, not a function returning these: spelled as a function (and as a
// structured binding of one) the same values gave other instruction schedules in up to half of the instantiations.
#define SEUNET_EPI_THREAD(LPV)                                \
  const int n = blockIdx.y, P = gridDim.x;                    \
  const int cg = threadIdx.x % LPV, vb = threadIdx.x / LPV;   \
  constexpr int VPB = EPI_THREADS / LPV;                      \
  const int c0 = cg * 8

// InstanceNorm + LeakyReLU of one value, and the LeakyReLU's derivative at the normalised value xh
__device__ __forceinline__ float lrelu(float xh, float slope) { return xh > 0.f ? xh : xh * slope; }
__device__ __forceinline__ float norm_lrelu(float x, float mu, float rs, float slope) { return lrelu((x - mu) * rs, slope); }
__device__ __forceinline__ float lrelu_slope(float xh, float slope) { return xh > 0.f ? 1.f : slope; }

// ---- fixed-order block sums: what makes every statistic bitwise reproducible ---------------------------------------------
// The four waves' values of one slot, summed in wave order: of a per-channel record red[wave][group][k], of a per-scalar
// one red[wave][k], of a single value w[wave].
template <typename E, int K> __device__ __forceinline__ E wave4_sum(const E (&red)[4][16][K], int g, int k) {
  return ((red[0][g][k] + red[1][g][k]) + red[2][g][k]) + red[3][g][k];
}
template <typename E, int K> __device__ __forceinline__ E wave4_sum(const E (&red)[4][K], int k) {
  return ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}
template <typename E> __device__ __forceinline__ E wave4_sum(const E (&w)[4]) { return ((w[0] + w[1]) + w[2]) + w[3]; }

// Per-scalar block sum of K values per thread: wave butterfly, one slot per wave, barrier; wave4_sum(red, k) is then the
// block's sum of value k.
template <int K> __device__ __forceinline__ void block_sum(const double (&s)[K], double (&red)[4][K]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double r = s[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) r += shfl_xor_settled(r, off);
    if (lane == 0) red[wave][k] = r;
  }
  __syncthreads();
}

// one 256-thread block per (n, c): sums the f64 partial slots in a fixed order.
//   mode 0: (mean, rstd = 1/sqrt(biased var + eps))      [InstanceNorm3d forward]
//   mode 1: (sum/count, sumsq/count)                     [the two means of the InstanceNorm backward]
// (stats_finalize_kernel, epilogue.hip, and the first blocks of gate_bwd_finalize_kernel, gate.hip)
__device__ __forceinline__ void stats_finalize_body(int idx, const double* __restrict__ partial, int slots, int C, double inv_count,
                                                    float eps, int mode, float* __restrict__ out_a, float* __restrict__ out_b) {
  const int n = idx / C, c = idx % C;
  double s1 = 0.0, s2 = 0.0;
  for (int p = threadIdx.x; p < slots; p += 256) {
    const double* q = partial + (((long long)n * slots + p) * C + c) * 2;
    s1 += q[0];
    s2 += q[1];
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    s1 += shfl_xor_settled(s1, off);
    s2 += shfl_xor_settled(s2, off);
  }
  __shared__ double w1[4], w2[4];
  if ((threadIdx.x & 63) == 0) { w1[threadIdx.x >> 6] = s1; w2[threadIdx.x >> 6] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    s1 = wave4_sum(w1);
    s2 = wave4_sum(w2);
    if (mode == 0) {
      const double mean = s1 * inv_count;
      double var = s2 * inv_count - mean * mean;
      if (var < 0.0) var = 0.0;
      out_a[idx] = (float)mean;
      out_b[idx] = (float)(1.0 / sqrt(var + (double)eps));
    } else {
      out_a[idx] = (float)(s1 * inv_count);
      out_b[idx] = (float)(s2 * inv_count);
    }
  }
}

// ---- launcher helpers ------------------------------------------------------------------------------------------------
#define SEUNET_LPV_SWITCH(LPVVAL, ...)                                                  \
  switch (LPVVAL) {                                                                       \
    case 1: { constexpr int LPV = 1; __VA_ARGS__; } break;                                       \
    case 2: { constexpr int LPV = 2; __VA_ARGS__; } break;                                       \
    case 4: { constexpr int LPV = 4; __VA_ARGS__; } break;                                       \
    case 8: { constexpr int LPV = 8; __VA_ARGS__; } break;                                       \
    case 16: { constexpr int LPV = 16; __VA_ARGS__; } break;                                     \
    default: return fail("unsupported channel count %d (need 8,16,32,64 or 128)", (LPVVAL)*8); \
  }

static int check_c(int C) {
  SEUNET_CHECK(C % 8 == 0 && C >= 8 && C <= 128 && (C & (C - 1)) == 0, "channel count %d must be a power of two in [8,128]", C);
  return 0;
}
#endif  // __HIPCC__

}  // namespace seunet
