// Kernels of the bit-packed volume layer (bitvol.h): byte <-> bit packing and the exclusive scan.
#include "bitvol.h"

namespace seunet {

namespace {

// bytes -> bits: one wave per word, lane j reads voxel 64 w + j of the row (coalesced), the ballot is the word.  PAIR: a second
// mask packed in the same launch.  PAIR and PAD are template arguments: with run-time tests of b and g.pad this kernel took 263
// against the 239 us of the kernel it replaced at 512^3, as templates 247 us.
template <bool PAIR, bool PAD>
__global__ void __launch_bounds__(256)
pack_bits_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, BitGeom g, u64* __restrict__ out_a,
                 u64* __restrict__ out_b) {
  const long long t = (blockIdx.x * 256ll + threadIdx.x) >> 6;      // wave-uniform
  if (t >= g.words) return;                                          // whole wavefronts leave together
  const int lane = threadIdx.x & 63;
  const int w = (int)(t % g.W);
  const long long row = t / g.W;
  const int k = w * 64 + lane;
  const bool in = k < g.n2;
  const long long v = row * g.n2 + k;
  const u64 ma = __ballot(in && a[v] != 0), mb = PAIR ? __ballot(in && b[v] != 0) : 0ull;
  if (lane == 0) {
    const long long p = PAD ? padded_index(g, row, w) : t;
    out_a[p] = ma;
    if (PAIR) out_b[p] = mb;
  }
}

// bits -> bytes: one thread per voxel, the form of the morphology and the double threshold before the layer.  The wave-per-word
// form of the thinning put binary_dilation at 512^3 outside the parent's spread; the thinning's own time holds with this one
// (DESIGN.md section 3n has both measurements).
template <bool PAD>
__global__ void __launch_bounds__(256) unpack_bits_kernel(const u64* __restrict__ bits, BitGeom g, long long n, unsigned char* __restrict__ out) {
  const long long idx = blockIdx.x * 256ll + threadIdx.x;
  if (idx >= n) return;
  const long long row = idx / g.n2;
  const int k = (int)(idx % g.n2);
  const long long p = PAD ? padded_index(g, row, k >> 6) : row * g.W + (k >> 6);
  out[idx] = (unsigned char)((bits[p] >> (k & 63)) & 1ull);
}

// Exclusive scan of every block of kScanBlock elements in place; the block's total to blk.  `b` / `blk_b`: a second array scanned
// in the same launch (null: none).
__global__ void __launch_bounds__(256)
scan_block_kernel(unsigned* __restrict__ a, unsigned* __restrict__ b, long long n, unsigned* __restrict__ blk_a,
                  unsigned* __restrict__ blk_b) {
  __shared__ unsigned sh[2][256];
  const int tid = threadIdx.x;
  const long long at = blockIdx.x * (long long)kScanBlock + tid * 4;
  for (int which = 0; which < 2; ++which) {
    unsigned* p = which ? b : a;
    if (!p) break;                                           // uniform
    unsigned v[4], sum = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[q] = at + q < n ? p[at + q] : 0u;
      sum += v[q];
    }
    sh[0][tid] = sum;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < 256; off <<= 1) {                // Hillis-Steele, double-buffered
      sh[cur ^ 1][tid] = sh[cur][tid] + (tid >= off ? sh[cur][tid - off] : 0u);
      cur ^= 1;
      __syncthreads();
    }
    unsigned run = sh[cur][tid] - sum;                       // exclusive
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (at + q < n) p[at + q] = run;
      run += v[q];
    }
    if (tid == 255) (which ? blk_b : blk_a)[blockIdx.x] = sh[cur][255];
    __syncthreads();
  }
}

// One workgroup: exclusive scan of the block totals in place (32 bits kept: an index the callers use fits, see the launchers'
// checks), the grand totals in 64 bits to total[0] (a) and total[1] (b).
__global__ void __launch_bounds__(1024)
scan_top_kernel(unsigned* __restrict__ blk_a, unsigned* __restrict__ blk_b, long long nb, u64* __restrict__ total) {
  __shared__ u64 sh[2][1024];
  __shared__ u64 carry;
  const int tid = threadIdx.x;
  for (int which = 0; which < 2; ++which) {
    unsigned* p = which ? blk_b : blk_a;
    if (!p) break;
    if (tid == 0) carry = 0ull;
    __syncthreads();
    for (long long c = 0; c < nb; c += 1024) {
      const u64 v = c + tid < nb ? (u64)p[c + tid] : 0ull;
      sh[0][tid] = v;
      __syncthreads();
      int cur = 0;
      for (int off = 1; off < 1024; off <<= 1) {
        sh[cur ^ 1][tid] = sh[cur][tid] + (tid >= off ? sh[cur][tid - off] : 0ull);
        cur ^= 1;
        __syncthreads();
      }
      const u64 before = carry;
      if (c + tid < nb) p[c + tid] = (unsigned)(before + sh[cur][tid] - v);
      __syncthreads();                                       // everyone has read carry
      if (tid == 1023) carry = before + sh[cur][1023];
      __syncthreads();
    }
    if (tid == 0) total[which] = carry;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256)
scan_add_kernel(const unsigned* __restrict__ a, const unsigned* __restrict__ blk, long long n, const u64* __restrict__ total,
                unsigned* __restrict__ out) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i < n) out[i] = a[i] + blk[i / kScanBlock];
  else if (i == n) out[n] = (unsigned)total[0];
}

}  // namespace

void pack_bits(const unsigned char* a, const unsigned char* b, const BitGeom& g, u64* out_a, u64* out_b, hipStream_t s) {
  auto* kernel = b ? (g.pad ? pack_bits_kernel<true, true> : pack_bits_kernel<true, false>)
                   : (g.pad ? pack_bits_kernel<false, true> : pack_bits_kernel<false, false>);
  kernel<<<(unsigned)((g.words + 3) / 4), 256, 0, s>>>(a, b, g, out_a, out_b);
}

void unpack_bits(const u64* bits, const BitGeom& g, unsigned char* out, hipStream_t s) {
  const long long n = (long long)g.n0 * g.n1 * g.n2;
  auto* kernel = g.pad ? unpack_bits_kernel<true> : unpack_bits_kernel<false>;
  kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(bits, g, n, out);
}

int run_scan(unsigned* a, unsigned* b, long long n, unsigned* blk_a, unsigned* blk_b, u64* total, hipStream_t s) {
  const long long nb = (n + kScanBlock - 1) / kScanBlock;
  if (nb > 0) scan_block_kernel<<<(unsigned)nb, 256, 0, s>>>(a, b, n, blk_a, blk_b);
  scan_top_kernel<<<1, 1024, 0, s>>>(blk_a, blk_b, nb, total);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

void scan_add(const unsigned* a, const unsigned* blk, long long n, const u64* total, unsigned* out, hipStream_t s) {
  scan_add_kernel<<<(unsigned)((n + 1 + 255) / 256), 256, 0, s>>>(a, blk, n, total, out);
}

}  // namespace seunet
