// Airway tree parsing on the device: the ATM'22 branch labelling behind the BD metric.
//
// Reference (CPU, numpy / scipy.ndimage):
//   atm22_skel_parse.py:83-101   skeleton_parsing: 3x3x3 sum of the skeleton (ndimage.convolve, mode 'reflect') * skeleton; voxels
//                                with a sum above 3 (self + more than two neighbours) are branch points and removed; ndimage.label
//                                with the full 3x3x3 structure; components under 5 voxels removed; labelled AGAIN
//   atm22_skel_parse.py:103-108  tree_parsing_func: feature transform of EDT(1 - skeleton_parse); cd[inds] * label
//   atm22_skel_parse.py:110-135  loc_trachea (voxel counts per label), adjacent_map (6-adjacency between labels)
//   tree_parsing.py:148-159      the refinement loop: every step replaces one label value by another, so it runs on the host on
//                                the counts and the adjacency of the first volume, and one look-up pass applies it (prep.py)
// scipy numbers components in raster order of their first voxel, and the union-find of components.hip labels a component with
// its minimum linear index, so scipy's number = rank of the root among the roots.  Removing whole components leaves the others as
// they are: the second labelling is the rank among the roots that survive.  Ranks come from a prefix sum over the volume (block
// counts, one scan, in-block ballots): no atomic decides an order, the result is deterministic.
// Integer / index work: results are bit-identical to the reference (tests/test_parse_gpu.py against tests/golden/parse_known.npz).
#include "volume.h"
#include <algorithm>

namespace seunet {

// ---- skeleton_parsing ---------------------------------------------------------------------------------------------------

// keep[i] = skeleton voxel whose 3x3x3 sum (centre included, mode 'reflect': count27_clamped) is at most 3
__global__ void __launch_bounds__(256)
branch_point_kernel(const unsigned char* __restrict__ skel, int n0, int n1, int n2, unsigned char* __restrict__ keep) {
  const long long n = (long long)n0 * n1 * n2;
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  if (skel[i] == 0) { keep[i] = 0; return; }
  keep[i] = count27_clamped(skel, vox3(i, n1, n2), n0, n1, n2) <= 3 ? 1 : 0;
}

__device__ __forceinline__ bool surviving_root(const int* L, const unsigned int* cnt, long long i, long long n, int min_voxels) {
  return i < n && L[i] == (int)i && cnt[i] >= (unsigned int)min_voxels;
}

// surviving roots per block of 256 voxels
__global__ void __launch_bounds__(256)
root_count_kernel(const int* __restrict__ L, const unsigned int* __restrict__ cnt, long long n, int min_voxels,
                  unsigned int* __restrict__ block_roots) {
  __shared__ unsigned int w[4];
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  const u64 m = __ballot(surviving_root(L, cnt, i, n, min_voxels));
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = (unsigned int)__builtin_popcountll(m);
  __syncthreads();
  if (threadIdx.x == 0) block_roots[blockIdx.x] = w[0] + w[1] + w[2] + w[3];
}

// exclusive prefix sum of block_roots in place, one workgroup; total -> *num
__global__ void __launch_bounds__(1024)
root_scan_kernel(unsigned int* __restrict__ block_roots, long long nb, int* __restrict__ num) {
  __shared__ unsigned int part[1024];
  const long long chunk = (nb + 1023) / 1024;
  const long long lo = std::min<long long>(threadIdx.x * chunk, nb), hi = std::min<long long>(lo + chunk, nb);
  unsigned int sum = 0;
  for (long long k = lo; k < hi; ++k) sum += block_roots[k];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {         // inclusive scan of the 1024 chunk sums
    const unsigned int add = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0u;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  unsigned int run = part[threadIdx.x] - sum;
  for (long long k = lo; k < hi; ++k) {
    const unsigned int c = block_roots[k];
    block_roots[k] = run;
    run += c;
  }
  if (threadIdx.x == 1023 && num) *num = (int)part[1023];
}

// cnt[root] := the component's number (1-based rank among the surviving roots), 0 for a removed one.  Every lane touches only
// its own entry.
__global__ void __launch_bounds__(256)
root_number_kernel(const int* __restrict__ L, unsigned int* __restrict__ cnt, long long n, int min_voxels,
                   const unsigned int* __restrict__ block_prefix) {
  __shared__ unsigned int w[4];
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool root = i < n && L[i] == (int)i;
  const bool keep = root && cnt[i] >= (unsigned int)min_voxels;
  const u64 m = __ballot(keep);
  if (lane == 0) w[wave] = (unsigned int)__builtin_popcountll(m);
  __syncthreads();
  if (!root) return;
  unsigned int before = block_prefix[blockIdx.x];
  for (int k = 0; k < wave; ++k) before += w[k];
  before += (unsigned int)__builtin_popcountll(m & ((1ull << lane) - 1ull));
  cnt[i] = keep ? before + 1u : 0u;
}

__global__ void __launch_bounds__(256)
branch_number_kernel(const int* __restrict__ L, const unsigned int* __restrict__ number, long long n, int* __restrict__ cd,
                     unsigned char* __restrict__ parse) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const int r = L[i];
  const int v = r >= 0 ? (int)number[r] : 0;
  cd[i] = v;
  if (parse) parse[i] = v ? 1 : 0;
}

size_t skeleton_branches_workspace_bytes(int n0, int n1, int n2) { return measured(branches_ws, n0, n1, n2); }

int launch_skeleton_branches(const unsigned char* skel, int n0, int n1, int n2, int min_voxels, int* cd, unsigned char* skeleton_parse,
                             int* num_dev, void* workspace, size_t ws_bytes, hipStream_t s) {
  SEUNET_CHECK(skel && cd && workspace, "skeleton_branches: null argument");
  if (volume_check("skeleton_branches", n0, n1, n2, 0)) return 1;
  SEUNET_CHECK(min_voxels >= 0, "skeleton_branches: min_voxels %d", min_voxels);
  WsCarver carve(workspace);
  const BranchesWs w = branches_ws(carve, n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "skeleton_branches: workspace too small");
  const long long n = (long long)n0 * n1 * n2;
  const unsigned blocks = blocks_256(n);
  SEUNET_HIP(hipMemsetAsync(w.counts, 0, (size_t)n * 4, s));
  branch_point_kernel<<<blocks, 256, 0, s>>>(skel, n0, n1, n2, w.keep);
  cc_label26(w.keep, n0, n1, n2, w.labels, s);
  launch_cc_count(w.labels, n, w.counts, s);
  root_count_kernel<<<blocks, 256, 0, s>>>(w.labels, w.counts, n, min_voxels, w.block_roots);
  root_scan_kernel<<<1, 1024, 0, s>>>(w.block_roots, (long long)blocks, num_dev);
  root_number_kernel<<<blocks, 256, 0, s>>>(w.labels, w.counts, n, min_voxels, w.block_roots);
  branch_number_kernel<<<blocks, 256, 0, s>>>(w.labels, w.counts, n, cd, skeleton_parse);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// ---- tree_parsing_func ----------------------------------------------------------------------------------------------------
// The feature transform of edt.hip with the sites = the voxels of skeleton_parse; its last pass gathers cd at the nearest site
// instead of storing the (3, n0, n1, n2) index volume.

size_t parse_assign_workspace_bytes(int n0, int n1, int n2) { return edt_workspace_bytes(n0, n1, n2); }

int launch_parse_assign(const unsigned char* skeleton_parse, const int* cd, const unsigned char* label, int n0, int n1, int n2,
                        int* parsing, int* status_dev, void* workspace, size_t ws_bytes, hipStream_t s) {
  SEUNET_CHECK(skeleton_parse && cd && label && parsing && workspace, "parse_assign: null argument");
  EdtOut o{};
  o.gather_src = cd;
  o.gather_mask = label;
  o.gather_out = parsing;
  return run_edt(skeleton_parse, true, n0, n1, n2, o, status_dev, workspace, ws_bytes, s);
}

// ---- label statistics -------------------------------------------------------------------------------------------------------

constexpr int kStatsBins = 4096;          // labels 0 .. 4095: one LDS histogram per workgroup (16 KB)

__device__ __forceinline__ void adjacency_set(u64* __restrict__ bits, int words, int a, int b) {
  u64* w = bits + (size_t)a * words + (b >> 6);
  const u64 bit = 1ull << (b & 63);
  if ((*w & bit) == 0) atomicOr(w, bit);          // a stale read only costs one more atomic
}

__global__ void __launch_bounds__(256)
label_stats_kernel(const int* __restrict__ parsing, int n0, int n1, int n2, int num, unsigned int* __restrict__ counts,
                   u64* __restrict__ bits, int words, int* __restrict__ status) {
  __shared__ unsigned int hist[kStatsBins];
  for (int k = threadIdx.x; k <= num; k += 256) hist[k] = 0u;
  __syncthreads();
  const long long plane = (long long)n1 * n2, n = (long long)n0 * plane;
  const int lane = threadIdx.x & 63;
  for (long long base = blockIdx.x * 256ll; base < n; base += (long long)gridDim.x * 256) {
    const long long i = base + threadIdx.x;
    int a = -1;
    if (i < n) {
      a = parsing[i];
      if (a < 0 || a > num) { *status = 1; a = -1; }
    }
    // one LDS atomic per run of equal labels inside a wave (components.hip, cc_count_kernel)
    const int prev = dpp_settle(__shfl_up(a, 1, 64));
    const bool lead = a >= 0 && (lane == 0 || prev != a);
    const u64 leaders = __ballot(lead), in = __ballot(a >= 0);
    if (lead) {
      const u64 after = (lane == 63) ? 0ull : ((leaders | ~in) >> (lane + 1));
      const int len = after ? __builtin_ctzll(after) + 1 : 64 - lane;
      atomicAdd(&hist[a], (unsigned int)len);
    }
    if (a > 0) {
      const Vox3 p = vox3(i, n1, n2);
      const int i0 = p.i0, i1 = p.i1, i2 = p.i2;
      int nb[3] = {0, 0, 0};
      if (i2 + 1 < n2) nb[0] = parsing[i + 1];
      if (i1 + 1 < n1) nb[1] = parsing[i + n2];
      if (i0 + 1 < n0) nb[2] = parsing[i + plane];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int b = nb[q];
        if (b > 0 && b <= num && b != a) { adjacency_set(bits, words, a, b); adjacency_set(bits, words, b, a); }
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k <= num; k += 256)
    if (hist[k]) atomicAdd(&counts[k], hist[k]);
}

int label_stats_max_num() { return kStatsBins - 1; }

int launch_label_stats(const int* parsing, int n0, int n1, int n2, int num, unsigned int* counts, u64* adjacency_bits, int* status_dev,
                       hipStream_t s) {
  SEUNET_CHECK(parsing && counts && adjacency_bits && status_dev, "label_stats: null argument");
  if (volume_check("label_stats", n0, n1, n2, 0)) return 1;
  SEUNET_CHECK(num >= 0 && num <= label_stats_max_num(), "label_stats: num %d: labels 0 .. %d are supported", num, label_stats_max_num());
  const long long n = (long long)n0 * n1 * n2;
  const int words = (num + 1 + 63) / 64;
  SEUNET_HIP(hipMemsetAsync(counts, 0, (size_t)(num + 1) * 4, s));
  SEUNET_HIP(hipMemsetAsync(adjacency_bits, 0, (size_t)(num + 1) * words * 8, s));
  SEUNET_HIP(hipMemsetAsync(status_dev, 0, sizeof(int), s));
  const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 2048);
  label_stats_kernel<<<blocks, 256, 0, s>>>(parsing, n0, n1, n2, num, counts, adjacency_bits, words, status_dev);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// ---- relabel ------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
relabel_kernel(const int* parsing, long long n, const int* __restrict__ lut, int nlut, int* out) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const int v = parsing[i];
  out[i] = (v >= 0 && v < nlut) ? lut[v] : 0;
}

int launch_relabel(const int* parsing, long long n, const int* lut, int nlut, int* out, hipStream_t s) {
  SEUNET_CHECK(parsing && lut && out && n >= 1 && nlut >= 1, "relabel: bad argument");
  SEUNET_CHECK(n < (1ll << 31) * 256, "relabel: %lld elements", n);
  relabel_kernel<<<blocks_256(n), 256, 0, s>>>(parsing, n, lut, nlut, out);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// ---- the reference's own parser: what its host graph stage asks of the device -------------------------

// out[0..2] += count, sum of i0, sum of i1 over the non-zero voxels of slice [:, :, k]
__global__ void __launch_bounds__(256)
slice_moments_kernel(const unsigned char* __restrict__ mask, int n0, int n1, int n2, int k, u64* __restrict__ out) {
  const long long rows = (long long)n0 * n1;
  u64 cnt = 0, s0 = 0, s1 = 0;
  for (long long r = blockIdx.x * 256ll + threadIdx.x; r < rows; r += (long long)gridDim.x * 256) {
    if (mask[r * n2 + k] != 0) {
      cnt += 1;
      s0 += (u64)(r / n1);
      s1 += (u64)(r % n1);
    }
  }
  cnt = wave_sum(cnt); s0 = wave_sum(s0); s1 = wave_sum(s1);
  if ((threadIdx.x & 63) == 0 && cnt) {
    atomicAdd(&out[0], cnt);
    atomicAdd(&out[1], s0);
    atomicAdd(&out[2], s1);
  }
}

int launch_slice_moments(const unsigned char* mask, int n0, int n1, int n2, int k, unsigned long long* out_dev, hipStream_t s) {
  SEUNET_CHECK(mask && out_dev, "slice_moments: null argument");
  if (volume_check("slice_moments", n0, n1, n2, 0)) return 1;
  SEUNET_CHECK(k >= 0 && k < n2, "slice_moments: slice %d of an axis of %d", k, n2);
  SEUNET_HIP(hipMemsetAsync(out_dev, 0, 3 * sizeof(u64), s));
  slice_moments_kernel<<<grid_for((long long)n0 * n1), 256, 0, s>>>(mask, n0, n1, n2, k, out_dev);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// cd[lin[j]] = value[j], skeleton_parse[lin[j]] = value[j] != 0; an index outside 0 .. n - 1 sets *status and is skipped.  The
// caller passes every voxel once, so no order among the lanes decides anything.
__global__ void __launch_bounds__(256)
scatter_labels_kernel(const long long* __restrict__ lin, const int* __restrict__ value, long long m, long long n, int* __restrict__ cd,
                      unsigned char* __restrict__ parse, int* __restrict__ status) {
  const long long j = blockIdx.x * 256ll + threadIdx.x;
  if (j >= m) return;
  const long long i = lin[j];
  if (i < 0 || i >= n) { *status = 1; return; }
  const int v = value[j];
  cd[i] = v;
  parse[i] = v != 0 ? 1 : 0;
}

int launch_scatter_labels(const long long* lin_index, const int* value, long long m, long long n, int* cd, unsigned char* skeleton_parse,
                          int* status_dev, hipStream_t s) {
  SEUNET_CHECK(cd && skeleton_parse && status_dev && m >= 0 && n >= 1, "scatter_labels: bad argument");
  SEUNET_CHECK(m == 0 || (lin_index && value), "scatter_labels: null list");
  SEUNET_CHECK(m < (1ll << 31) * 256, "scatter_labels: %lld entries", m);
  SEUNET_HIP(hipMemsetAsync(status_dev, 0, sizeof(int), s));
  if (m > 0) scatter_labels_kernel<<<blocks_256(m), 256, 0, s>>>(lin_index, value, m, n, cd, skeleton_parse, status_dev);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
