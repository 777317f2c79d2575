// CT preprocessing on the device: value counts, HU shift + padding clamp, the per-slice lung field, the bounding box and crops
// (reference preprocessing.py:26-130 with util.py:95-165).
//
//   value counts   cnt[(uint16)(int16)(v + shift)] for every voxel: the host builds the reference's 300-bin histograms from them
//                  (np.histogram over the distinct values with the counts as weights gives the same edges and bins)
//   shift + clamp  out = (int16)(v + 1024), then `case_pixels[case_pixels <= -800] = aaa` (preprocessing.py:47, :69-71)
//   get_l          util.py:120-152 for every processed slice n (axis 2) at once: threshold, largest 8-connected component,
//                  its 4-connected holes (2-D binary_fill_holes), the holes relabelled 8-connected, the two largest written
//                  when they have more than min_area pixels
//   box / crops    preprocessing.py:81-104 (the margin arithmetic is the caller's)
//
// The per-slice labelling is the union-find of components.hip (cc_find / cc_union, volume.h) restricted to in-plane
// neighbours: lanes run along the contiguous axis 2, so a wave holds up to 64 different slices at one (i, j), every neighbour
// read (strides Z and W*Z) is coalesced, and no link ever crosses from one slice to another.  For a fixed n the minimum
// linear index of a component is the raster order of its first pixel (i, j), i.e. skimage's / scipy's label order, which is the
// tie rule of np.argmax over the bincounts.  The per-slice argmax is one 64-bit atomicMax of (count << 32) | ~root into a
// Z-entry array: the most pixels first, then the smallest root.  Integer work only: the result is deterministic.
#include "volume.h"
#include <algorithm>

namespace seunet {

// ---- value counts -----------------------------------------------------------------------------------------------------------
// One block counts LUNG_COUNT_CHUNK consecutive voxels into 65536 16-bit counters packed two to an LDS word (128 KiB); the chunk
// is below 65536 so no half-word carries into its neighbour.  Inside a wave, a run of equal values along the contiguous axis
// is one LDS atomic (the padding and air regions of a CT are long runs).  The block then adds its non-zero counters to the
// global uint32 counts.
constexpr int LUNG_COUNT_THREADS = 1024;
constexpr int LUNG_COUNT_ITERS = 63;
constexpr long long LUNG_COUNT_CHUNK = (long long)LUNG_COUNT_THREADS * LUNG_COUNT_ITERS;   // 64512 < 65536
static_assert(LUNG_COUNT_CHUNK < 65536, "per-block counts must fit 16 bits");

__global__ void __launch_bounds__(LUNG_COUNT_THREADS)
lung_value_count_kernel(const short* __restrict__ ct, long long n, int shift, unsigned int* __restrict__ cnt) {
  __shared__ unsigned int bins[32768];
  for (int w = threadIdx.x; w < 32768; w += LUNG_COUNT_THREADS) bins[w] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const long long base = blockIdx.x * LUNG_COUNT_CHUNK;
  for (int it = 0; it < LUNG_COUNT_ITERS; ++it) {
    const long long i = base + (long long)it * LUNG_COUNT_THREADS + threadIdx.x;
    const bool in = i < n;
    const int v = in ? (int)(unsigned short)(short)(ct[i] + shift) : -1;
    const int prev = dpp_settle(__shfl_up(v, 1, 64));
    const bool lead = in && (lane == 0 || prev != v);
    const u64 leaders = __ballot(lead), valid = __ballot(in);
    if (lead) {
      const u64 after = (lane == 63) ? 0ull : ((leaders | ~valid) >> (lane + 1));
      const unsigned len = after ? (unsigned)__builtin_ctzll(after) + 1u : 64u - (unsigned)lane;
      atomicAdd(&bins[v >> 1], len << ((v & 1) * 16));
    }
  }
  __syncthreads();
  for (int w = threadIdx.x; w < 32768; w += LUNG_COUNT_THREADS) {
    const unsigned b = bins[w];
    if (b & 0xffffu) atomicAdd(&cnt[2 * w], b & 0xffffu);
    if (b >> 16) atomicAdd(&cnt[2 * w + 1], b >> 16);
  }
}

int launch_value_counts(const short* ct, long long n, int shift, unsigned int* counts, hipStream_t s) {
  SEUNET_CHECK(ct && counts && n >= 1, "value_counts: bad argument");
  SEUNET_HIP(hipMemsetAsync(counts, 0, 65536 * sizeof(unsigned int), s));
  const long long blocks = (n + LUNG_COUNT_CHUNK - 1) / LUNG_COUNT_CHUNK;
  SEUNET_CHECK(blocks < (1ll << 31), "value_counts: %lld voxels is too many", n);
  lung_value_count_kernel<<<(unsigned)blocks, LUNG_COUNT_THREADS, 0, s>>>(ct, n, shift, counts);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// ---- shift + padding clamp --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
lung_shift_clamp_kernel(const short* __restrict__ ct, long long n, int shift, int clamp, int clamp_le, short clamp_to,
                        short* __restrict__ out) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  short v = (short)(ct[i] + shift);                   // int16 arithmetic of numpy: wraps
  if (clamp && v <= clamp_le) v = clamp_to;
  out[i] = v;
}

int launch_shift_clamp(const short* ct, long long n, int shift, int clamp, int clamp_le, int clamp_to, short* out, hipStream_t s) {
  SEUNET_CHECK(ct && out && n >= 1, "shift_clamp: bad argument");
  SEUNET_CHECK(clamp_to >= -32768 && clamp_to <= 32767, "shift_clamp: clamp value %d is not an int16", clamp_to);
  lung_shift_clamp_kernel<<<blocks_256(n), 256, 0, s>>>(ct, n, shift, clamp, clamp_le, (short)clamp_to, out);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// ---- get_l: the lung field of every processed slice -------------------------------------------------------------------------
// util.py:123: for n in range(int(0.05 * Z) - 1, int(0.95 * Z)); n = -1 (Z < 20) is the last slice.
struct SliceRange { int lo, hi, last; };
static SliceRange get_l_range(int Z) {
  const int first = (int)(0.05 * Z) - 1, end = (int)(0.95 * Z);
  SliceRange r;
  r.lo = first < 0 ? 0 : first;
  r.hi = end;
  r.last = first < 0;
  return r;
}
__device__ __forceinline__ bool slice_processed(int z, int Z, SliceRange r) { return (z >= r.lo && z < r.hi) || (r.last && z == Z - 1); }

// L[i] = i where the processed slice has ct >= T (compared in float64, util.py:128), -1 elsewhere
__global__ void __launch_bounds__(256)
lung_threshold_kernel(const short* __restrict__ ct, long long n, int Z, double T, SliceRange r, int* __restrict__ L) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const int z = (int)(i % Z);
  L[i] = (slice_processed(z, Z, r) && (double)ct[i] >= T) ? (int)i : -1;
}

// in-plane links to the neighbours that precede pixel (x, y) in raster order: 4 of the 8 (CONN8) or 2 of the 4
template <bool CONN8>
__global__ void __launch_bounds__(256)
lung_merge_kernel(int* L, long long n, int W, int Z) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  if (L[i] < 0) return;
  const Vox3 p = vox3(i, W, Z);
  const int x = p.i0, y = p.i1;
  const long long sx = (long long)W * Z;
  if (y > 0 && L[i - Z] >= 0) cc_union(L, (int)i, (int)(i - Z));
  if (x > 0) {
    if (L[i - sx] >= 0) cc_union(L, (int)i, (int)(i - sx));
    if (CONN8) {
      if (y > 0 && L[i - sx - Z] >= 0) cc_union(L, (int)i, (int)(i - sx - Z));
      if (y < W - 1 && L[i - sx + Z] >= 0) cc_union(L, (int)i, (int)(i - sx + Z));
    }
  }
}

// pixel count per root (roots of neighbouring lanes lie in different slices: no wave aggregation)
__global__ void __launch_bounds__(256)
lung_count_kernel(const int* __restrict__ L, long long n, unsigned int* __restrict__ cnt) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const int r = L[i];
  if (r >= 0) atomicAdd(&cnt[r], 1u);
}

__device__ __forceinline__ u64 slice_key(unsigned c, int root) { return ((u64)c << 32) | (u64)(~(unsigned)root); }
__device__ __forceinline__ int key_root(u64 k) { return (int)~(unsigned)(k & 0xffffffffull); }
__device__ __forceinline__ unsigned key_count(u64 k) { return (unsigned)(k >> 32); }

// per slice: best[z] = max key over the roots of slice z (EXCLUDE: other than exclude[z])
template <bool EXCLUDE>
__global__ void __launch_bounds__(256)
lung_select_kernel(const int* __restrict__ L, const unsigned int* __restrict__ cnt, long long n, int Z, const u64* __restrict__ exclude,
                   u64* __restrict__ best) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n || L[i] != (int)i) return;
  const int z = (int)(i % Z);
  const u64 key = slice_key(cnt[i], (int)i);
  if (EXCLUDE && key == exclude[z]) return;
  atomicMax(&best[z], key);
}

// complement of img1 (the largest component) in the processed slices: the background that binary_fill_holes examines.
// A slice without foreground has img1 = imLabel == 0 (the background itself, util.py:131-133): it is filled whole, no holes.
__global__ void __launch_bounds__(256)
lung_complement_kernel(int* L, long long n, int Z, SliceRange r, const u64* __restrict__ best) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const int z = (int)(i % Z);
  const u64 b = best[z];
  L[i] = (slice_processed(z, Z, r) && b != 0 && L[i] != key_root(b)) ? (int)i : -1;
}

// background components (4-connected) with a pixel on the slice border are not holes
__global__ void __launch_bounds__(256)
lung_border_kernel(const int* __restrict__ L, long long n, int H, int W, int Z, unsigned int* __restrict__ flag) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const Vox3 p = vox3(i, W, Z);
  const int x = p.i0, y = p.i1;
  if (!(x == 0 || x == H - 1 || y == 0 || y == W - 1)) return;
  if (L[i] >= 0) flag[L[i]] = 1u;
}

// img3 = img1 ^ binary_fill_holes(img1): the enclosed background pixels
__global__ void __launch_bounds__(256)
lung_holes_kernel(int* L, long long n, const unsigned int* __restrict__ flag) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const int r = L[i];
  L[i] = (r >= 0 && flag[r] == 0u) ? (int)i : -1;
}

// L[:, :, n] = img11 (max_num1 > min_area) | img22 (max_num2 > min_area); unprocessed slices stay 0
__global__ void __launch_bounds__(256)
lung_write_kernel(const int* __restrict__ L, long long n, int Z, const u64* __restrict__ top1, const u64* __restrict__ top2,
                  unsigned min_area, unsigned char* __restrict__ out) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const int z = (int)(i % Z), r = L[i];
  const u64 a = top1[z], b = top2[z];
  const bool in1 = a != 0 && key_count(a) > min_area && r == key_root(a);
  const bool in2 = b != 0 && key_count(b) > min_area && r == key_root(b);
  out[i] = (r >= 0 && (in1 || in2)) ? 1 : 0;
}

size_t get_l_workspace_bytes(int H, int W, int Z) { return measured(get_l_ws, H, W, Z); }

int launch_get_l(const short* ct, int H, int W, int Z, double T, int min_area, unsigned char* out, void* workspace, size_t ws_bytes,
                 hipStream_t s) {
  SEUNET_CHECK(ct && out && workspace && H >= 1 && W >= 1 && Z >= 1 && min_area >= 0, "get_l: bad argument");
  if (volume_check("get_l", H, W, Z, 0, true)) return 1;
  WsCarver carve(workspace);
  const GetLWs w = get_l_ws(carve, H, W, Z);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "get_l: workspace too small");
  const long long n = (long long)H * W * Z;
  int* L = w.labels;
  unsigned int* cnt = w.counts;
  u64 *best = w.best, *top1 = w.top1, *top2 = w.top2;
  const SliceRange r = get_l_range(Z);
  const unsigned blocks = blocks_256(n);
  SEUNET_HIP(hipMemsetAsync(cnt, 0, (size_t)n * 4, s));
  SEUNET_HIP(hipMemsetAsync(best, 0, w.key_bytes, s));          // best, top1 and top2
  // img1: the largest 8-connected component of ct >= T per slice (skimage's measure.label default connectivity in 2-D)
  lung_threshold_kernel<<<blocks, 256, 0, s>>>(ct, n, Z, T, r, L);
  lung_merge_kernel<true><<<blocks, 256, 0, s>>>(L, n, W, Z);
  launch_cc_compress(L, n, s);
  lung_count_kernel<<<blocks, 256, 0, s>>>(L, n, cnt);
  lung_select_kernel<false><<<blocks, 256, 0, s>>>(L, cnt, n, Z, nullptr, best);
  // its holes: the 4-connected background components (binary_fill_holes' default cross) that do not reach the slice border
  lung_complement_kernel<<<blocks, 256, 0, s>>>(L, n, Z, r, best);
  SEUNET_HIP(hipMemsetAsync(cnt, 0, (size_t)n * 4, s));
  lung_merge_kernel<false><<<blocks, 256, 0, s>>>(L, n, W, Z);
  launch_cc_compress(L, n, s);
  lung_border_kernel<<<blocks, 256, 0, s>>>(L, n, H, W, Z, cnt);
  lung_holes_kernel<<<blocks, 256, 0, s>>>(L, n, cnt);
  // the holes relabelled 8-connected (holes touching at a corner merge), the two largest per slice
  SEUNET_HIP(hipMemsetAsync(cnt, 0, (size_t)n * 4, s));
  lung_merge_kernel<true><<<blocks, 256, 0, s>>>(L, n, W, Z);
  launch_cc_compress(L, n, s);
  lung_count_kernel<<<blocks, 256, 0, s>>>(L, n, cnt);
  lung_select_kernel<false><<<blocks, 256, 0, s>>>(L, cnt, n, Z, nullptr, top1);
  lung_select_kernel<true><<<blocks, 256, 0, s>>>(L, cnt, n, Z, top1, top2);
  lung_write_kernel<<<blocks, 256, 0, s>>>(L, n, Z, top1, top2, (unsigned)min_area, out);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// ---- two-mask combination and bounding box ----------------------------------------------------------------------------------
// op 0: out = (a != 0) ^ (b != 0) (preprocessing.py:78, L ^ L1); op 1: out = (a != 0) | (b != 0) (:79, L1 + L2 of bools)
__global__ void __launch_bounds__(256)
lung_combine_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, long long n, int op,
                    unsigned char* __restrict__ out) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const bool x = a[i] != 0, y = b[i] != 0;
  out[i] = (op == 0 ? (x != y) : (x || y)) ? 1 : 0;
}

int launch_mask_combine(const unsigned char* a, const unsigned char* b, long long n, int op, unsigned char* out, hipStream_t s) {
  SEUNET_CHECK(a && b && out && n >= 1, "mask_combine: bad argument");
  SEUNET_CHECK(op == 0 || op == 1, "mask_combine: op %d (0 = xor, 1 = or)", op);
  lung_combine_kernel<<<blocks_256(n), 256, 0, s>>>(a, b, n, op, out);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

__global__ void lung_box_init_kernel(int* box) {
  if (threadIdx.x < 6) box[threadIdx.x] = (threadIdx.x & 1) ? -1 : 0x7fffffff;
}

// box = {min x, max x, min y, max y, min z, max z} of the non-zero voxels; a wave reduces first, then six atomics
__global__ void __launch_bounds__(256)
lung_box_kernel(const unsigned char* __restrict__ mask, long long n, int W, int Z, int* __restrict__ box) {
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1};
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    if (!mask[i]) continue;
    const Vox3 p = vox3(i, W, Z);
    const int c[3] = {p.i0, p.i1, p.i2};
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], c[a]); hi[a] = max(hi[a], c[a]); }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      lo[a] = min(lo[a], shfl_xor_settled(lo[a], off));
      hi[a] = max(hi[a], shfl_xor_settled(hi[a], off));
    }
  }
  if ((threadIdx.x & 63) == 0 && hi[0] >= 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicMin(&box[2 * a], lo[a]); atomicMax(&box[2 * a + 1], hi[a]); }
  }
}

int launch_mask_box(const unsigned char* mask, int H, int W, int Z, int* box, hipStream_t s) {
  SEUNET_CHECK(mask && box && H >= 1 && W >= 1 && Z >= 1, "mask_box: bad argument");
  const long long n = (long long)H * W * Z;
  lung_box_init_kernel<<<1, 64, 0, s>>>(box);
  const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 4096);
  lung_box_kernel<<<blocks, 256, 0, s>>>(mask, n, W, Z, box);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// ---- crop: dst = src[x0:x1, y0:y1, z0:z1] (elements of 1 or 2 bytes) ----------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256)
lung_crop_kernel(const T* __restrict__ src, int W, int Z, int x0, int y0, int z0, int cw, int cz, long long m, T* __restrict__ dst) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= m) return;
  const Vox3 p = vox3(i, cw, cz);
  dst[i] = src[((long long)(x0 + p.i0) * W + (y0 + p.i1)) * Z + (z0 + p.i2)];
}

int launch_crop3d(const void* src, int elem_bytes, int H, int W, int Z, const int* box, void* dst, hipStream_t s) {
  SEUNET_CHECK(src && dst && box && H >= 1 && W >= 1 && Z >= 1, "crop3d: bad argument");
  SEUNET_CHECK(elem_bytes == 1 || elem_bytes == 2, "crop3d: %d-byte elements (1 or 2)", elem_bytes);
  const int ext[3] = {H, W, Z};
  for (int a = 0; a < 3; ++a)
    SEUNET_CHECK(box[2 * a] >= 0 && box[2 * a] < box[2 * a + 1] && box[2 * a + 1] <= ext[a], "crop3d: box [%d, %d) outside axis %d of %d",
                 box[2 * a], box[2 * a + 1], a, ext[a]);
  const int cw = box[3] - box[2], cz = box[5] - box[4];
  const long long m = (long long)(box[1] - box[0]) * cw * cz;
  const unsigned blocks = blocks_256(m);
  if (elem_bytes == 1)
    lung_crop_kernel<unsigned char><<<blocks, 256, 0, s>>>((const unsigned char*)src, W, Z, box[0], box[2], box[4], cw, cz, m,
                                                          (unsigned char*)dst);
  else
    lung_crop_kernel<short><<<blocks, 256, 0, s>>>((const short*)src, W, Z, box[0], box[2], box[4], cw, cz, m, (short*)dst);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
