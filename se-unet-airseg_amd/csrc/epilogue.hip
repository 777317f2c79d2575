// HBM-bound "epilogue" kernels of the SE-UNet blocks (gfx950): what the gated block (gate.hip) and the aggregation block
// (cat.hip) share -- the partial-record count of every pass, the per-(n,c) channel statistics and their finaliser.
// Thread mapping and the shared device steps: epilogue.h.
#include "epilogue.h"

namespace seunet {

int epi_partials(Dims d) {
  // One partial record per block and sample.  128 voxels per block at least: the coarse levels (32^3, 16^3) were running
  // pass A on 4..32 blocks per sample, 32 dependent iterations each (36 us for a 16^3 x 64-channel tensor).  256 at most
  // (every record is summed again by the finalize kernels: 512 made those 30 % slower for nothing).
  // Wave quantisation: pass A of the one-gate blocks holds 3 workgroups per CU (162 VGPRs), i.e. 768 on the chip; 4 x 256 =
  // 1024 blocks ran as one full round and a third of a second one.  The count per launch (N x partials; the other passes
  // use 4 x as many) is therefore rounded down to a multiple of 768 once it exceeds it: 4 x 192 at the bench shape, measured
  // against 96 / 160 / 224 / 256 / 384 per sample (sum of the epilogue classes 5.64 ms vs 6.12 / 5.90 / 5.99 / 5.83 / 5.86).
  long long v = d.vox();
  long long p = v / 128;
  if (p < 1) p = 1;
  if (p > 256) p = 256;
  const long long n = d.N > 0 ? d.N : 1, round = 3 * 256;
  if (n * p >= round) {
    const long long q = (n * p / round) * round / n;
    if (q >= 1) p = q;
  }
  return (int)p;
}

// ----------------------------------------------------------------------------------
// generic per-(n,c) sum / sum of squares of a channels-last tensor
// ----------------------------------------------------------------------------------
template <typename T, int LPV>
__global__ void __launch_bounds__(EPI_THREADS)
channel_stats_kernel(const T* __restrict__ t, int C, double* __restrict__ partial, long long V) {
  SEUNET_EPI_THREAD(LPV);
  double s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { s1[j] = 0.0; s2[j] = 0.0; }
  for (long long v = (long long)blockIdx.x * VPB + vb; v < V; v += (long long)P * VPB) {
    float x[8];
    load8(t + ((long long)n * V + v) * C + c0, x);
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] += (double)x[j]; s2[j] += (double)x[j] * (double)x[j]; }
  }
  __shared__ double red[4][16][16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    double a = stride_sum_d<LPV>(s1[j]), b = stride_sum_d<LPV>(s2[j]);
    if (lane < LPV) { red[wave][lane][j] = a; red[wave][lane][8 + j] = b; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < LPV * 16; i += EPI_THREADS) {
    const int g = i / 16, k = i % 16;
    const double tot = wave4_sum(red, g, k);
    const int c = g * 8 + (k & 7);
    partial[(((long long)n * P + blockIdx.x) * C + c) * 2 + (k >> 3)] = tot;
  }
}

__global__ void __launch_bounds__(256)
stats_finalize_kernel(const double* __restrict__ partial, int slots, int C, int N, double inv_count,
                      float eps, int mode, float* __restrict__ out_a, float* __restrict__ out_b) {
  stats_finalize_body(blockIdx.x, partial, slots, C, inv_count, eps, mode, out_a, out_b);
}

int launch_channel_stats(int dtype, const void* t, int C, double* partial, Dims d, hipStream_t s) {
  if (int e = check_c(C)) return e;
  dim3 grid(epi_partials(d), d.N);
  SEUNET_LPV_SWITCH(C / 8, {
    SEUNET_DTYPE_SWITCH(dtype, channel_stats_kernel<T, LPV><<<grid, EPI_THREADS, 0, s>>>((const T*)t, C, partial, d.vox()));
  });
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_stats_finalize(const double* partial, int slots, int C, int N, long long count, float eps,
                          int mode, float* out_a, float* out_b, hipStream_t s) {
  stats_finalize_kernel<<<N * C, 256, 0, s>>>(partial, slots, C, N, 1.0 / (double)count, eps, mode, out_a, out_b);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
