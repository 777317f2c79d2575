// Surface distances of two binary volumes on the device: the distances behind the Hausdorff distance, its percentiles, the average
// symmetric surface distance and the surface Dice at a tolerance.  The reference computes none of them; the
// definition is include/seunet_hip.h, restated in numpy by tests/surface_oracle.py.
//
//   count    both masks are bit-packed along axis 2 by one pack_bits launch (bitvol.h); one pass on the
//            packed words forms both border masks (set, and one of the six neighbours unset or outside: load_cross6 with outside
//            = 0), counts their bits per word and reduces the bounding box of A | B; run_scan scans the two count arrays in one
//            launch.  The host reads the two totals and the box once.
//   emit     per direction, inside the box only: the other mask's border becomes the zero voxels of a byte volume, the EDT with
//            spacing (edt_sampling.hip, as it is) gives every box voxel the linear index of its feature, and every border bit of
//            this mask writes sqrt((dt0^2 + dt1^2) + dt2^2) at the position the scan gives it: raster order, A's then B's.  All
//            sites and queries lie in the box and dt_a = (index_a - coordinate_a) * s_a depends on differences only, so each
//            distance is the one of the full volume bit for bit.  No distance volume is written.
//   summary  count, maximum (on the bit patterns), elements <= tolerance and the float64 sum per direction.  The sum is a tree of a
//            fixed shape: per-thread strided partials, wave butterfly, the block's four waves in order, then one block over the
//            block partials.  No atomics: the same bits on every run.
//   select   exact order statistics by a radix select on the 64-bit patterns (non-negative doubles order as their patterns): eight
//            passes of eight bits, most significant first.  Per pass one histogram per request in LDS (a wave whose hits share a digit adds
//            once), one integer atomic per non-empty bin and block, then a one-block step that picks the digit and updates prefix and remaining rank in device
//            memory.  Nothing returns to the host between passes.
#include "volume.h"
#include <cmath>

// the distances are numpy's float64 arithmetic operation by operation, as edt_sampling.hip's last pass and wall_step
#pragma clang fp contract(off)

namespace seunet {

namespace {

constexpr int kSummaryBlocks = 128;       // workgroups per direction of the summary's first pass; the second pass is one workgroup
constexpr int kSelectBits = 8;            // 256 bins x 8 requests x 4 bytes = 8 KB of LDS per workgroup
constexpr int kSelectBins = 1 << kSelectBits;
constexpr int kSelectPasses = 64 / kSelectBits;
constexpr int kSelectMaxBlocks = 512;

// ---- count -------------------------------------------------------------------------------------------------------------------
// the border bits of word idx: set, and not all six neighbours set (morph.hip's erosion with outside = 0, then x & ~eroded)
__device__ __forceinline__ u64 border_word(const u64* __restrict__ in, const BitGeom& g, long long idx) {
  const u64 x = in[idx];
  if (!x) return 0ull;
  return x & ~and6(load_cross6(in, g, idx, 0ull));
}

// one thread per word: both borders, their bit counts, and the box of A | B as six maxima (exclusive high ends, and extent - low
// end), so that a zeroed record is the empty box.  Wave and workgroup maxima first, then at most six integer atomics per workgroup (none for a workgroup of empty words).
__global__ void __launch_bounds__(256)
surface_border_kernel(const u64* __restrict__ pa, const u64* __restrict__ pb, BitGeom g, u64* __restrict__ ba, u64* __restrict__ bb,
                      unsigned* __restrict__ ca, unsigned* __restrict__ cb, SurfaceRec* __restrict__ rec) {
  __shared__ int part[4][6];
  const long long idx = blockIdx.x * 256ll + threadIdx.x;
  int v[6] = {0, 0, 0, 0, 0, 0};
  if (idx < g.words) {
    const long long row = idx / g.W;
    const int m = (int)(idx % g.W);
    const int i1 = (int)(row % g.n1), i0 = (int)(row / g.n1);
    const u64 xa = border_word(pa, g, idx), xb = border_word(pb, g, idx);
    ba[idx] = xa;
    bb[idx] = xb;
    ca[idx] = (unsigned)__popcll(xa);
    cb[idx] = (unsigned)__popcll(xb);
    const u64 any = pa[idx] | pb[idx];
    if (any) {
      v[0] = i0 + 1;
      v[1] = i1 + 1;
      v[2] = 64 * m + 64 - __clzll((long long)any);
      v[3] = g.n0 - i0;
      v[4] = g.n1 - i1;
      v[5] = g.n2 - (64 * m + __ffsll((unsigned long long)any) - 1);
    }
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) v[q] = wave_max(v[q]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < 6; ++q) part[threadIdx.x >> 6][q] = v[q];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int q = threadIdx.x;
    const int top = std::max(std::max(part[0][q], part[1][q]), std::max(part[2][q], part[3][q]));
    int* p = q < 3 ? &rec->hi[q] : &rec->from_end[q - 3];
    if (top > 0) atomicMax(p, top);
  }
}

// ---- emit --------------------------------------------------------------------------------------------------------------------
struct SurfaceBox { int lo[3], ext[3]; };

// the EDT's input on the box: 0 (a site) at the border voxels of the other mask, 1 elsewhere
__global__ void __launch_bounds__(256)
surface_sites_kernel(const u64* __restrict__ border, BitGeom g, SurfaceBox bx, long long nbox, unsigned char* __restrict__ sites) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= nbox) return;
  const Vox3 p = vox3(i, bx.ext[1], bx.ext[2]);
  const long long row = (long long)(p.i0 + bx.lo[0]) * g.n1 + (p.i1 + bx.lo[1]);
  const int k = p.i2 + bx.lo[2];
  sites[i] = (unsigned char)(((border[row * g.W + (k >> 6)] >> (k & 63)) & 1ull) ^ 1ull);
}

// one wave per word of the box's rows, lane j = bit j.  A border bit writes its distance at the position the scan gives it.
__global__ void __launch_bounds__(256)
surface_gather_kernel(const u64* __restrict__ border, const unsigned* __restrict__ cnt, const unsigned* __restrict__ blk, BitGeom g,
                      SurfaceBox bx, int w_lo, int w_span, long long items, const int* __restrict__ lin, double s0, double s1,
                      double s2, long long count, double* __restrict__ dist, int* __restrict__ voxel) {
  const long long t = (blockIdx.x * 256ll + threadIdx.x) >> 6;      // wave-uniform
  if (t >= items) return;
  const int lane = threadIdx.x & 63;
  const long long r = t / w_span;
  const int wi = (int)(t % w_span) + w_lo;
  const int c1 = (int)(r % bx.ext[1]), c0 = (int)(r / bx.ext[1]);      // box coordinates of the row
  const int i0 = c0 + bx.lo[0], i1 = c1 + bx.lo[1];
  const long long idx = ((long long)i0 * g.n1 + i1) * g.W + wi;
  const u64 bits = border[idx];
  if (!((bits >> lane) & 1ull)) return;
  const long long pos = (long long)cnt[idx] + blk[idx / kScanBlock] + __popcll(bits & ((1ull << lane) - 1ull));
  if (pos >= count) return;                                          // (cannot happen with the totals of the count pass)
  const int k = wi * 64 + lane, c2 = k - bx.lo[2];
  if (c2 < 0 || c2 >= bx.ext[2]) return;                             // (cannot happen with the box of the count pass)
  const int f = lin[((long long)c0 * bx.ext[1] + c1) * bx.ext[2] + c2];
  double d = HUGE_VAL;                                               // (no site: cannot happen, the other border is not empty)
  if (f >= 0) {
    const int j2 = f % bx.ext[2], fr = f / bx.ext[2];
    const int j1 = fr % bx.ext[1], j0 = fr / bx.ext[1];
    const double t0 = (double)(j0 - c0) * s0, t1 = (double)(j1 - c1) * s1, t2 = (double)(j2 - c2) * s2;
    d = sqrt((t0 * t0 + t1 * t1) + t2 * t2);
  }
  dist[pos] = d;
  if (voxel) voxel[pos] = (int)(((long long)i0 * g.n1 + i1) * g.n2 + k);
}

// ---- summary -----------------------------------------------------------------------------------------------------------------
struct SurfaceTol { double t[kSurfaceMaxTol]; int n; };

// words of the record and of one partial: sum, maximum, then the counts
__host__ __device__ constexpr int summary_part_words(int ntol) { return 2 + ntol; }
__host__ __device__ constexpr int summary_rec_words(int ntol) { return 2 * (3 + ntol); }

// the workgroup's reduction in a fixed order: butterfly inside each wave, then the four waves in ascending order (thread 0 holds
// the result)
__device__ __forceinline__ void summary_block_reduce(double& sum, u64& mx, u64 (&le)[kSurfaceMaxTol], int ntol) {
  __shared__ double s_sum[4];
  __shared__ u64 s_max[4], s_le[4][kSurfaceMaxTol];
  sum = wave_sum(sum);
  mx = wave_max(mx);
#pragma unroll
  for (int q = 0; q < kSurfaceMaxTol; ++q) {
    if (q < ntol) le[q] = wave_sum(le[q]);                           // uniform
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_sum[wave] = sum;
    s_max[wave] = mx;
#pragma unroll
    for (int q = 0; q < kSurfaceMaxTol; ++q)
      if (q < ntol) s_le[wave][q] = le[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    sum = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    mx = std::max(std::max(s_max[0], s_max[1]), std::max(s_max[2], s_max[3]));
#pragma unroll
    for (int q = 0; q < kSurfaceMaxTol; ++q)
      if (q < ntol) le[q] = s_le[0][q] + s_le[1][q] + s_le[2][q] + s_le[3][q];
  }
  __syncthreads();
}

// grid (kSummaryBlocks, 2): direction y; thread j of workgroup x takes elements x 256 + j + k 256 kSummaryBlocks, k = 0, 1, ...
__global__ void __launch_bounds__(256)
surface_summary_kernel(const double* __restrict__ dist, long long n_a, long long n_b, SurfaceTol tol, u64* __restrict__ partial) {
  const int dir = blockIdx.y;
  const double* p = dist + (dir ? n_a : 0);
  const long long n = dir ? n_b : n_a;
  double sum = 0.0;
  u64 mx = 0ull, le[kSurfaceMaxTol] = {};
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += 256ll * kSummaryBlocks) {
    const double d = p[i];
    sum += d;
    mx = std::max(mx, __builtin_bit_cast(u64, d));
#pragma unroll
    for (int q = 0; q < kSurfaceMaxTol; ++q)
      if (q < tol.n) le[q] += d <= tol.t[q] ? 1ull : 0ull;
  }
  summary_block_reduce(sum, mx, le, tol.n);
  if (threadIdx.x == 0) {
    u64* o = partial + ((long long)dir * kSummaryBlocks + blockIdx.x) * summary_part_words(tol.n);
    o[0] = __builtin_bit_cast(u64, sum);
    o[1] = mx;
#pragma unroll
    for (int q = 0; q < kSurfaceMaxTol; ++q)
      if (q < tol.n) o[2 + q] = le[q];
  }
}

// one workgroup: thread j takes the partial of workgroup j of the first pass.  rec: count[2], max[2], sum[2], le[2][ntol].
__global__ void __launch_bounds__(256)
surface_summary_top_kernel(const u64* __restrict__ partial, long long n_a, long long n_b, int ntol, u64* __restrict__ rec) {
  for (int dir = 0; dir < 2; ++dir) {
    double sum = 0.0;
    u64 mx = 0ull, le[kSurfaceMaxTol] = {};
    if (threadIdx.x < kSummaryBlocks) {
      const u64* o = partial + ((long long)dir * kSummaryBlocks + threadIdx.x) * summary_part_words(ntol);
      sum = __builtin_bit_cast(double, o[0]);
      mx = o[1];
#pragma unroll
      for (int q = 0; q < kSurfaceMaxTol; ++q)
        if (q < ntol) le[q] = o[2 + q];
    }
    summary_block_reduce(sum, mx, le, ntol);
    if (threadIdx.x == 0) {
      rec[dir] = (u64)(dir ? n_b : n_a);
      rec[2 + dir] = mx;
      rec[4 + dir] = __builtin_bit_cast(u64, sum);
#pragma unroll
      for (int q = 0; q < kSurfaceMaxTol; ++q)
        if (q < ntol) rec[6 + dir * ntol + q] = le[q];
    }
  }
}

// ---- select ------------------------------------------------------------------------------------------------------------------
struct SelectReq {
  long long begin[kSelectMaxRanks], end[kSelectMaxRanks], rank[kSelectMaxRanks];
  long long lo, hi;          // the span all segments lie in
  int n;
};

// histogram of this pass's digit per request, among the request's segment elements whose higher digits equal its prefix
__global__ void __launch_bounds__(256)
select_hist_kernel(const u64* __restrict__ bits, SelectReq q, int pass, const SelectState* __restrict__ st, unsigned* __restrict__ hist) {
  __shared__ unsigned lh[kSelectMaxRanks * kSelectBins];
  __shared__ u64 pre[kSelectMaxRanks];
  for (int j = threadIdx.x; j < q.n * kSelectBins; j += 256) lh[j] = 0u;
  if (threadIdx.x < q.n) pre[threadIdx.x] = pass ? st->prefix[threadIdx.x] : 0ull;
  __syncthreads();
  const int shift = 64 - kSelectBits * (pass + 1);
  const int lane = threadIdx.x & 63;
  for (long long base = q.lo + blockIdx.x * 256ll; base < q.hi; base += 256ll * gridDim.x) {      // uniform trip count
    const long long i = base + threadIdx.x;
    const bool in = i < q.hi;
    const u64 v = in ? bits[i] : 0ull;
    const u64 top = pass ? v >> (shift + kSelectBits) : 0ull;
    const int d = (int)((v >> shift) & (kSelectBins - 1));
#pragma unroll
    for (int r = 0; r < kSelectMaxRanks; ++r) {
      if (r >= q.n) break;                                           // uniform
      const bool hit = in && i >= q.begin[r] && i < q.end[r] && top == pre[r];
      const u64 who = __ballot(hit);
      if (!who) continue;                                            // uniform
      // the wave's partial first: where all its hits share one digit (ties, and the high digits of any data) one lane adds the
      // count; otherwise the hits are spread over bins and each adds its own
      const int leader = __ffsll(who) - 1;
      const int d0 = __builtin_amdgcn_readlane(d, leader);
      if (__ballot(hit && d == d0) == who) {
        if (lane == leader) atomicAdd(&lh[r * kSelectBins + d0], (unsigned)__popcll(who));
      } else if (hit) {
        atomicAdd(&lh[r * kSelectBins + d], 1u);
      }
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < q.n * kSelectBins; j += 256) {
    const unsigned c = lh[j];
    if (c) atomicAdd(&hist[j], c);
  }
}

// one workgroup, thread = bin: scan each request's histogram, the bin that holds the rank becomes the next digit of the prefix;
// the histogram is cleared for the next pass.  After the last pass the prefix is the value.
__global__ void __launch_bounds__(256)
select_step_kernel(SelectReq q, int pass, SelectState* __restrict__ st, unsigned* __restrict__ hist, double* __restrict__ out) {
  __shared__ u64 sh[2][kSelectBins];
  const int tid = threadIdx.x;
  for (int r = 0; r < q.n; ++r) {
    const u64 rank = pass ? st->rank[r] : (u64)q.rank[r];
    const u64 prefix = pass ? st->prefix[r] : 0ull;
    const u64 c = hist[r * kSelectBins + tid];
    hist[r * kSelectBins + tid] = 0u;
    sh[0][tid] = c;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < kSelectBins; off <<= 1) {                // Hillis-Steele, double-buffered
      sh[cur ^ 1][tid] = sh[cur][tid] + (tid >= off ? sh[cur][tid - off] : 0ull);
      cur ^= 1;
      __syncthreads();
    }
    const u64 incl = sh[cur][tid], excl = incl - c;
    if (c && excl <= rank && rank < incl) {                          // one thread: the bins partition the ranks
      const u64 next = (prefix << kSelectBits) | (u64)tid;
      st->prefix[r] = next;
      st->rank[r] = rank - excl;
      if (pass == kSelectPasses - 1) out[r] = __builtin_bit_cast(double, next);
    }
    __syncthreads();
  }
}

int check_spacing(const char* what, double s0, double s1, double s2) {
  SEUNET_CHECK(s0 > 0.0 && s1 > 0.0 && s2 > 0.0 && s0 < HUGE_VAL && s1 < HUGE_VAL && s2 < HUGE_VAL,
               "%s: the spacing must be three positive finite numbers, got (%g, %g, %g)", what, s0, s1, s2);
  return 0;
}

}  // namespace

size_t surface_workspace_bytes(int n0, int n1, int n2) { return measured(surface_ws, n0, n1, n2); }
size_t surface_emit_workspace_bytes(int b0, int b1, int b2) { return measured(surface_emit_ws, b0, b1, b2); }
size_t surface_summary_bytes(int ntol) {
  return sizeof(u64) * ((size_t)summary_rec_words(ntol) + 2 * (size_t)kSummaryBlocks * summary_part_words(ntol));
}
size_t select_ranks_workspace_bytes(int nranks) {
  WsCarver c(nullptr);
  select_ws(c, nranks);
  return c.bytes();
}

int launch_surface_count(const unsigned char* a, const unsigned char* b, int n0, int n1, int n2, long long* n_a, long long* n_b, int* box,
                         void* workspace, size_t ws_bytes, hipStream_t s) {
  SEUNET_CHECK(a && b && n_a && n_b && box && workspace, "surface_count: null argument");
  if (int e = volume_check("surface_count", n0, n1, n2, kEdtMaxExtent)) return e;
  WsCarver carve(workspace);
  const SurfaceWs w = surface_ws(carve, n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "surface_count: workspace too small (%zu bytes, %zu needed)", ws_bytes, carve.bytes());
  const BitGeom g = bit_geom(n0, n1, n2);
  SEUNET_HIP(hipMemsetAsync(w.rec, 0, sizeof(SurfaceRec), s));
  pack_bits(a, b, g, w.bits_a, w.bits_b, s);
  surface_border_kernel<<<blocks_256(g.words), 256, 0, s>>>(w.bits_a, w.bits_b, g, w.border_a, w.border_b, w.cnt_a, w.cnt_b, w.rec);
  if (int e = run_scan(w.cnt_a, w.cnt_b, g.words, w.blk_a, w.blk_b, &w.rec->n_a, s)) return e;
  SurfaceRec host;                                             // the one synchronisation: the output sizes and the box
  SEUNET_HIP(hipMemcpyAsync(&host, w.rec, sizeof(SurfaceRec), hipMemcpyDeviceToHost, s));
  SEUNET_HIP(hipStreamSynchronize(s));
  *n_a = (long long)host.n_a;
  *n_b = (long long)host.n_b;
  const int ext[3] = {n0, n1, n2};
  for (int q = 0; q < 3; ++q) {
    box[2 * q] = ext[q] - host.from_end[q];                    // an empty pair of masks: low = the extent, high = 0
    box[2 * q + 1] = host.hi[q];
  }
  return 0;
}

int launch_surface_emit(int n0, int n1, int n2, const int* box, double s0, double s1, double s2, long long n_a, long long n_b,
                        double* dist, int* voxel, const void* count_workspace, size_t count_bytes, void* emit_workspace, size_t emit_bytes,
                        hipStream_t s) {
  SEUNET_CHECK(box && dist && count_workspace && emit_workspace, "surface_emit: null argument");
  if (int e = volume_check("surface_emit", n0, n1, n2, kEdtMaxExtent)) return e;
  if (int e = check_spacing("surface_emit", s0, s1, s2)) return e;
  const int ext[3] = {n0, n1, n2};
  SurfaceBox bx;
  for (int q = 0; q < 3; ++q) {
    SEUNET_CHECK(box[2 * q] >= 0 && box[2 * q] < box[2 * q + 1] && box[2 * q + 1] <= ext[q],
                 "surface_emit: box [%d, %d) along axis %d is empty or outside the volume", box[2 * q], box[2 * q + 1], q);
    bx.lo[q] = box[2 * q];
    bx.ext[q] = box[2 * q + 1] - box[2 * q];
  }
  SEUNET_CHECK(n_a >= 1 && n_b >= 1, "surface_emit: %lld and %lld surface voxels: a mask without voxels has no surface distances",
               n_a, n_b);
  SEUNET_CHECK(n_a + n_b <= 0x7fffffffll, "surface_emit: %lld distances exceed the int32 range", n_a + n_b);
  WsCarver carve(const_cast<void*>(count_workspace));
  const SurfaceWs w = surface_ws(carve, n0, n1, n2);
  SEUNET_CHECK(count_bytes >= carve.bytes(), "surface_emit: count workspace too small (%zu bytes, %zu needed)", count_bytes, carve.bytes());
  WsCarver ecarve(emit_workspace);
  const SurfaceEmitWs e = surface_emit_ws(ecarve, bx.ext[0], bx.ext[1], bx.ext[2]);
  SEUNET_CHECK(emit_bytes >= ecarve.bytes(), "surface_emit: emit workspace too small (%zu bytes, %zu needed)", emit_bytes, ecarve.bytes());
  const BitGeom g = bit_geom(n0, n1, n2);
  const long long nbox = (long long)bx.ext[0] * bx.ext[1] * bx.ext[2];
  const int w_lo = bx.lo[2] / 64, w_span = (bx.lo[2] + bx.ext[2] - 1) / 64 - w_lo + 1;
  const long long items = (long long)bx.ext[0] * bx.ext[1] * w_span;
  for (int dir = 0; dir < 2; ++dir) {                          // 0: A's border against B's, 1: the mirror image
    const u64* mine = dir ? w.border_b : w.border_a;
    const u64* other = dir ? w.border_a : w.border_b;
    surface_sites_kernel<<<blocks_256(nbox), 256, 0, s>>>(other, g, bx, nbox, e.sites);
    if (int err = launch_edt_sampling(e.sites, bx.ext[0], bx.ext[1], bx.ext[2], s0, s1, s2, EdtSamplingOut{nullptr, nullptr, e.lin}, nullptr,
                                      e.edt.f0, e.edt_bytes, s))
      return err;
    surface_gather_kernel<<<(unsigned)((items + 3) / 4), 256, 0, s>>>(mine, dir ? w.cnt_b : w.cnt_a, dir ? w.blk_b : w.blk_a, g, bx,
                                                                     w_lo, w_span, items, e.lin, s0, s1, s2, dir ? n_b : n_a,
                                                                     dist + (dir ? n_a : 0), voxel ? voxel + (dir ? n_a : 0) : nullptr);
  }
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_surface_summary(const double* dist, long long n_a, long long n_b, const double* tol, int ntol, void* out_dev, hipStream_t s) {
  SEUNET_CHECK(out_dev, "surface_summary: null argument");
  SEUNET_CHECK(n_a >= 0 && n_b >= 0, "surface_summary: negative size");
  SEUNET_CHECK(dist || n_a + n_b == 0, "surface_summary: null distances");
  SEUNET_CHECK(ntol >= 0 && ntol <= kSurfaceMaxTol, "surface_summary: %d tolerances: 0 .. %d are supported", ntol, kSurfaceMaxTol);
  SEUNET_CHECK(ntol == 0 || tol, "surface_summary: null tolerances");
  SurfaceTol t{};
  t.n = ntol;
  for (int q = 0; q < ntol; ++q) t.t[q] = tol[q];
  u64* rec = reinterpret_cast<u64*>(out_dev);
  u64* partial = rec + summary_rec_words(ntol);
  surface_summary_kernel<<<dim3(kSummaryBlocks, 2), 256, 0, s>>>(dist, n_a, n_b, t, partial);
  surface_summary_top_kernel<<<1, 256, 0, s>>>(partial, n_a, n_b, ntol, rec);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_select_ranks(const double* values, long long n, const long long* seg_begin, const long long* seg_end, const long long* rank,
                        int nranks, double* out_dev, void* workspace, size_t ws_bytes, hipStream_t s) {
  SEUNET_CHECK(values && seg_begin && seg_end && rank && out_dev && workspace, "select_ranks: null argument");
  SEUNET_CHECK(nranks >= 1 && nranks <= kSelectMaxRanks, "select_ranks: %d requests: 1 .. %d are supported", nranks, kSelectMaxRanks);
  SEUNET_CHECK(n >= 1 && n <= 0x7fffffffll, "select_ranks: %lld values: 1 .. 2^31 - 1 are supported", n);
  SelectReq q{};
  q.n = nranks;
  q.lo = n;
  q.hi = 0;
  for (int r = 0; r < nranks; ++r) {
    SEUNET_CHECK(seg_begin[r] >= 0 && seg_begin[r] < seg_end[r] && seg_end[r] <= n,
                 "select_ranks: request %d: segment [%lld, %lld) is empty or outside the %lld values", r, seg_begin[r], seg_end[r], n);
    SEUNET_CHECK(rank[r] >= 0 && rank[r] < seg_end[r] - seg_begin[r], "select_ranks: request %d: rank %lld outside a segment of %lld", r,
                 rank[r], seg_end[r] - seg_begin[r]);
    q.begin[r] = seg_begin[r];
    q.end[r] = seg_end[r];
    q.rank[r] = rank[r];
    q.lo = std::min(q.lo, seg_begin[r]);
    q.hi = std::max(q.hi, seg_end[r]);
  }
  WsCarver carve(workspace);
  const SelectWs w = select_ws(carve, nranks);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "select_ranks: workspace too small (%zu bytes, %zu needed)", ws_bytes, carve.bytes());
  SEUNET_HIP(hipMemsetAsync(w.hist, 0, sizeof(unsigned) * (size_t)nranks * kSelectBins, s));
  const unsigned blocks = (unsigned)std::min<long long>((q.hi - q.lo + 1023) / 1024, kSelectMaxBlocks);
  for (int pass = 0; pass < kSelectPasses; ++pass) {
    select_hist_kernel<<<blocks, 256, 0, s>>>(reinterpret_cast<const u64*>(values), q, pass, w.state, w.hist);
    select_step_kernel<<<1, 256, 0, s>>>(q, pass, w.state, w.hist, out_dev);
  }
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
