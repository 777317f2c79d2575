// Branch morphometry on the device: the integer tables behind per-branch length, volume and radius.
//
// The reference measures nothing per branch; the definition is the one of include/seunet_hip.h (seunet_branch_stats), restated in
// plain numpy by tests/morphometry_oracle.py.  From a `parsing` volume (int32, values 0 .. num), the `skeleton` mask and the integer
// squared EDT, for every label: voxels, coordinate sums, bounding box; skeleton voxels, links between neighbouring skeleton voxels
// by offset class, and the sum / minimum / maximum of the squared distance over its skeleton voxels.
//
// Two streaming passes and one table initialisation, none of them per label:
//   volume pass    every workgroup reads one contiguous chunk of `parsing`.  A run of equal labels inside a wave and inside a row
//                  (label_stats_kernel's idiom, cut at row starts so that i0 and i1 are constant and i2 is an arithmetic series) is
//                  added by its first lane alone: four sums and a box in closed form.  The sums go to an LDS table of kLdsSlots rows,
//                  slot = label modulo kLdsSlots, owned by the first label to claim it and flushed once per workgroup; a label that
//                  finds its slot taken by another goes to the global tables directly (a chunk is a few rows of a few slices and
//                  meets few labels, so that is rare).  Background costs a load.
//   skeleton pass  reads `skeleton`, 16 bytes per lane; `parsing`, `sqdist` and the 26 neighbours are touched at set voxels only.  A
//                  wave sums what its lanes hold for one label with ballots and settled shuffles, and its first lane of that label
//                  adds the sums.
// Everything is integer: sums are 64-bit, minima and maxima are atomicMin / atomicMax, so no order of execution shows in a result.
#include "volume.h"
#include <algorithm>
#include <climits>

namespace seunet {

constexpr int kLdsSlots = 256;            // rows of the LDS table: 256 x (4 + 4 x 8 + 6 x 4) = 15 KB per workgroup, so that the 8
                                          // workgroups per CU of the volume pass are resident together
constexpr int kTilesInFlight = 4;         // tiles of 256 voxels a workgroup of the volume pass loads before it uses the first
constexpr int kLinkClasses = 13;          // the offsets of {-1, 0, 1}^3 lexicographically above (0, 0, 0)
constexpr int kVolumeBlocks = 2048;       // workgroups of the volume pass: 8 per CU

// The 3x3x3 block around a voxel, cell (d0 + 1) * 9 + (d1 + 1) * 3 + (d2 + 1): ascending cells are ascending lexicographic
// offsets, the centre is cell 13 and link class c is cell 14 + c.
// Cells a link of cell `cell` is checked against: the centre plus every proper non-empty subset of the offset's non-zero components.
__host__ __device__ constexpr unsigned link_shortcut_cells(int cell) {
  const int d[3] = {cell / 9 - 1, cell / 3 % 3 - 1, cell % 3 - 1};
  const int step[3] = {9, 3, 1};
  int full = 0;
  for (int a = 0; a < 3; ++a) full |= d[a] != 0 ? 1 << a : 0;
  unsigned cells = 0;
  for (int sub = 1; sub < 8; ++sub) {
    if ((sub & full) != sub || sub == full) continue;
    int at = 13;
    for (int a = 0; a < 3; ++a)
      if (sub >> a & 1) at += d[a] * step[a];
    cells |= 1u << at;
  }
  return cells;
}
static_assert(link_shortcut_cells(14) == 0, "a face link has no shortcut");
static_assert(__builtin_popcount(link_shortcut_cells(15)) == 2 && __builtin_popcount(link_shortcut_cells(26)) == 6,
              "an edge diagonal has 2 intermediate voxels, a corner diagonal 6");

// ---- table initialisation: rows 0 .. num to their empty values ---------------------------------------------------------------
__global__ void __launch_bounds__(256)
branch_stats_init_kernel(BranchStatsOut o, int n0, int n1, int n2, int num) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k == 0) *o.status = 0;
  if (k > num) return;
  o.voxels[k] = 0;
  o.skeleton_voxels[k] = 0;
  o.r2_sum[k] = 0;
  o.r2_min[k] = INT_MAX;
  o.r2_max[k] = -1;
  const int ext[3] = {n0, n1, n2};
  for (int a = 0; a < 3; ++a) {
    o.coord_sum[3 * k + a] = 0;
    o.box_min[3 * k + a] = ext[a];
    o.box_max[3 * k + a] = -1;
  }
  for (int c = 0; c < kLinkClasses; ++c) {
    o.links[kLinkClasses * k + c] = 0;
    o.cross_links[kLinkClasses * k + c] = 0;
  }
}

// ---- volume pass ----------------------------------------------------------------------------------------------------------------

// lowers *p to v / raises it to v; the values only move one way, so a stale read costs one more atomic and nothing else
__device__ __forceinline__ void lower_to(int* p, int v) { if (*p > v) atomicMin(p, v); }
__device__ __forceinline__ void raise_to(int* p, int v) { if (*p < v) atomicMax(p, v); }

// one table set: the global one (row = label) or a workgroup's LDS table (row = slot)
struct VolumeTables { u64 *cnt, *sum; int *lo, *hi; };

__device__ __forceinline__ void add_row(const VolumeTables& t, int a, u64 cnt, u64 s0, u64 s1, u64 s2, const int (&lo)[3], const int (&hi)[3]) {
  atomicAdd(&t.cnt[a], cnt);
  if (s0) atomicAdd(&t.sum[3 * a + 0], s0);
  if (s1) atomicAdd(&t.sum[3 * a + 1], s1);
  if (s2) atomicAdd(&t.sum[3 * a + 2], s2);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    lower_to(&t.lo[3 * a + q], lo[q]);
    raise_to(&t.hi[3 * a + q], hi[q]);
  }
}

// chunk: voxels per workgroup, a multiple of 256, so that a wave covers the same 64 voxels whatever the grid
__global__ void __launch_bounds__(256)
branch_volume_kernel(const int* __restrict__ parsing, int n0, int n1, int n2, int num, long long chunk, BranchStatsOut o) {
  __shared__ u64 s_cnt[kLdsSlots], s_sum[3 * kLdsSlots];
  __shared__ int s_lo[3 * kLdsSlots], s_hi[3 * kLdsSlots];
  __shared__ int s_owner[kLdsSlots];                       // the label a slot belongs to, 0: free; set once (0 -> label), never changed
  for (int k = threadIdx.x; k < kLdsSlots; k += 256) { s_cnt[k] = 0; s_owner[k] = 0; }
  for (int k = threadIdx.x; k < 3 * kLdsSlots; k += 256) { s_sum[k] = 0; s_lo[k] = INT_MAX; s_hi[k] = -1; }
  __syncthreads();
  const VolumeTables lds{s_cnt, s_sum, s_lo, s_hi};
  const VolumeTables global{reinterpret_cast<u64*>(o.voxels), reinterpret_cast<u64*>(o.coord_sum), o.box_min, o.box_max};
  const long long n = (long long)n0 * n1 * n2;
  const long long begin = blockIdx.x * chunk, end = std::min(begin + chunk, n);
  const int lane = threadIdx.x & 63;
  for (long long tile = begin; tile < end; tile += kTilesInFlight * 256) {
    int loaded[kTilesInFlight];                            // the loads of kTilesInFlight tiles are issued before the first is used
#pragma unroll
    for (int u = 0; u < kTilesInFlight; ++u) {
      const long long i = tile + u * 256 + threadIdx.x;
      loaded[u] = i < end ? parsing[i] : 0;
    }
#pragma unroll
    for (int u = 0; u < kTilesInFlight; ++u) {
      const long long i = tile + u * 256 + threadIdx.x;
      int a = loaded[u];
      if (a < 0 || a > num) { *o.status = 1; a = 0; }
      // one set of atomics per run of equal labels inside a wave (label_stats_kernel), cut at the start of a row; background skipped
      const int prev = dpp_settle(__shfl_up(a, 1, 64));
      bool lead = false;
      Vox3 p{};
      if (a > 0) {
        p = vox3(i, n1, n2);
        lead = lane == 0 || prev != a || p.i2 == 0;
      }
      const u64 leaders = __ballot(lead), fg = __ballot(a > 0);
      if (lead) {
        const u64 after = (lane == 63) ? 0ull : ((leaders | ~fg) >> (lane + 1));
        const u64 len = after ? __builtin_ctzll(after) + 1 : 64 - lane;      // 1 .. 64 voxels (i0, i1, i2 .. i2 + len - 1)
        const int lo[3] = {p.i0, p.i1, p.i2}, hi[3] = {p.i0, p.i1, p.i2 + (int)len - 1};
        const u64 s0 = len * (u64)p.i0, s1 = len * (u64)p.i1, s2 = len * (u64)p.i2 + len * (len - 1) / 2;
        const int slot = a & (kLdsSlots - 1);
        int owner = __hip_atomic_load(&s_owner[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (owner == 0) {                                  // free when read: claim it; whoever wins, the slot has an owner afterwards
          owner = atomicCAS(&s_owner[slot], 0, a);
          if (owner == 0) owner = a;
        }
        if (owner == a) add_row(lds, slot, len, s0, s1, s2, lo, hi);
        else add_row(global, a, len, s0, s1, s2, lo, hi);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kLdsSlots; k += 256) {
    if (s_owner[k] == 0) continue;
    const int lo[3] = {s_lo[3 * k], s_lo[3 * k + 1], s_lo[3 * k + 2]}, hi[3] = {s_hi[3 * k], s_hi[3 * k + 1], s_hi[3 * k + 2]};
    add_row(global, s_owner[k], s_cnt[k], s_sum[3 * k], s_sum[3 * k + 1], s_sum[3 * k + 2], lo, hi);
  }
}

// ---- skeleton pass ----------------------------------------------------------------------------------------------------------------

// lanes set in `m`, as a 64-bit count
__device__ __forceinline__ u64 lanes(u64 m) { return (u64)__builtin_popcountll(m); }

// what the skeleton pass adds to
struct SkeletonTables { u64 *skeleton_voxels, *links, *cross_links, *r2_sum; int *r2_min, *r2_max; };

// One voxel per lane, i valid where `set`; called by whole waves (the ballots and shuffles below need every lane).
__device__ __forceinline__ void skeleton_step(const int* __restrict__ parsing, const unsigned char* __restrict__ skel,
                                              const int* __restrict__ sqdist, int n0, int n1, int n2, int num, long long i, bool set,
                                              const SkeletonTables& t) {
  const long long plane = (long long)n1 * n2;
  const int lane = threadIdx.x & 63;
  int a = 0;
  if (set) {
    a = parsing[i];
    if (a < 1 || a > num) a = 0;
  }
  if (__ballot(a > 0) == 0) return;                      // (wave-uniform) skeleton voxels of label 0 only
  unsigned same = 0, cross = 0;                          // bit c: a counted link of class c to the same / to another label
  int r2 = 0;
  if (a > 0) {
    const Vox3 p = vox3(i, n1, n2);
    // the 26 skeleton bytes first, from addresses that are legal whatever the cell (a cell outside the volume reads the centre), so
    // that the loads do not wait for each other; `parsing` then only where a byte is set
    unsigned near = 0;                                   // bit `cell`: inside the volume and on the skeleton
#pragma unroll
    for (int cell = 0; cell < 27; ++cell) {
      if (cell == 13) continue;
      const int d0 = cell / 9 - 1, d1 = cell / 3 % 3 - 1, d2 = cell % 3 - 1;
      const int x0 = p.i0 + d0, x1 = p.i1 + d1, x2 = p.i2 + d2;
      const bool inside = x0 >= 0 && x0 < n0 && x1 >= 0 && x1 < n1 && x2 >= 0 && x2 < n2;
      if (skel[inside ? i + d0 * plane + d1 * n2 + d2 : i] != 0 && inside) near |= 1u << cell;
    }
    unsigned occupied = 0;                               // bit `cell`: a labelled skeleton voxel there
    int nb[kLinkClasses];                                // labels of the 13 forward neighbours
#pragma unroll
    for (int cell = 0; cell < 27; ++cell) {
      if (cell == 13) continue;
      const int d0 = cell / 9 - 1, d1 = cell / 3 % 3 - 1, d2 = cell % 3 - 1;
      int b = 0;
      if (near >> cell & 1u) {
        b = parsing[i + d0 * plane + d1 * n2 + d2];
        if (b < 1 || b > num) b = 0;
      }
      if (b) occupied |= 1u << cell;
      if (cell > 13) nb[cell - 14] = b;
    }
#pragma unroll
    for (int c = 0; c < kLinkClasses; ++c) {
      if (nb[c] == 0 || (occupied & link_shortcut_cells(14 + c)) != 0) continue;
      if (nb[c] == a) same |= 1u << c;
      else {                                             // the other label's share; this one's goes through the wave sum below
        cross |= 1u << c;
        atomicAdd(&t.cross_links[kLinkClasses * nb[c] + c], 1ull);
      }
    }
    if (sqdist) r2 = sqdist[i];
  }
  // wave-uniform from here: one label of the wave at a time, summed over the lanes that hold it
  u64 pending = __ballot(a > 0);
  while (pending) {
    const int first = __builtin_ctzll(pending);
    const int label = dpp_settle(__shfl(a, first, 64));
    const bool mine = a == label;
    const u64 holders = __ballot(mine);
    u64 n_same[kLinkClasses], n_cross[kLinkClasses];     // at most 64 each: lanes of one wave
#pragma unroll
    for (int c = 0; c < kLinkClasses; ++c) {
      n_same[c] = lanes(__ballot(mine && (same >> c & 1u)));
      n_cross[c] = lanes(__ballot(mine && (cross >> c & 1u)));
    }
    u64 sum = 0;
    int lo = INT_MAX, hi = -1;
    if (sqdist) {                                        // (wave-uniform)
      sum = mine ? (u64)(long long)r2 : 0ull;
      lo = mine ? r2 : INT_MAX;
      hi = mine ? r2 : INT_MIN;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        sum += shfl_xor_settled(sum, off);
        lo = std::min(lo, shfl_xor_settled(lo, off));
        hi = std::max(hi, shfl_xor_settled(hi, off));
      }
    }
    if (lane == first) {
      atomicAdd(&t.skeleton_voxels[label], lanes(holders));
#pragma unroll
      for (int c = 0; c < kLinkClasses; ++c) {
        if (n_same[c]) atomicAdd(&t.links[kLinkClasses * label + c], n_same[c]);
        if (n_cross[c]) atomicAdd(&t.cross_links[kLinkClasses * label + c], n_cross[c]);
      }
      if (sqdist) {
        if (sum) atomicAdd(&t.r2_sum[label], sum);
        lower_to(&t.r2_min[label], lo);
        raise_to(&t.r2_max[label], hi);
      }
    }
    pending &= ~holders;
  }
}

// A lane loads 16 bytes of the skeleton at once, from 16-byte aligned addresses: with `skew` = the address of skel modulo 16,
// byte j of the aligned stream is voxel j - skew.  A wave leaves its 1024 bytes at once when none is set, which is the rule.
__global__ void __launch_bounds__(256)
branch_skeleton_kernel(const int* __restrict__ parsing, const unsigned char* __restrict__ skel, const int* __restrict__ sqdist, int n0,
                       int n1, int n2, int num, int skew, BranchStatsOut o) {
  const long long n = (long long)n0 * n1 * n2, stream = n + skew;
  const unsigned char* const aligned = skel - skew;
  const SkeletonTables t{reinterpret_cast<u64*>(o.skeleton_voxels), reinterpret_cast<u64*>(o.links), reinterpret_cast<u64*>(o.cross_links),
                         reinterpret_cast<u64*>(o.r2_sum), o.r2_min, o.r2_max};
  for (long long base = blockIdx.x * 4096ll; base < stream; base += (long long)gridDim.x * 4096) {
    const long long at = base + 16ll * threadIdx.x;
    u64 half[2] = {0ull, 0ull};
    if (at >= skew && at + 16 <= stream) {
      const uint4 w = *reinterpret_cast<const uint4*>(aligned + at);
      half[0] = (u64)w.y << 32 | w.x;
      half[1] = (u64)w.w << 32 | w.z;
    } else {                                             // the ends of the volume: byte by byte, nothing outside it is read
      for (int b = 0; b < 16; ++b)
        if (at + b >= skew && at + b < stream) half[b >> 3] |= (u64)aligned[at + b] << (8 * (b & 7));
    }
    if (__ballot((half[0] | half[1]) != 0) == 0) continue;   // (wave-uniform)
#pragma unroll 1
    for (int b = 0; b < 16; ++b) {
      const bool set = ((b < 8 ? half[0] : half[1]) >> (8 * (b & 7)) & 0xffull) != 0;
      if (__ballot(set) == 0) continue;                  // (wave-uniform)
      skeleton_step(parsing, skel, sqdist, n0, n1, n2, num, at + b - skew, set, t);
    }
  }
}

int launch_branch_stats(const int* parsing, const unsigned char* skeleton, const int* sqdist, int n0, int n1, int n2, int num,
                        BranchStatsOut o, hipStream_t s) {
  SEUNET_CHECK(parsing && skeleton && o.voxels && o.coord_sum && o.box_min && o.box_max && o.skeleton_voxels && o.links &&
                   o.cross_links && o.r2_sum && o.r2_min && o.r2_max && o.status,
               "branch_stats: null argument");
  if (volume_check("branch_stats", n0, n1, n2, 0)) return 1;
  SEUNET_CHECK(num >= 0 && num <= label_stats_max_num(), "branch_stats: num %d: labels 0 .. %d are supported", num, label_stats_max_num());
  const long long n = (long long)n0 * n1 * n2;
  branch_stats_init_kernel<<<blocks_256(num + 1), 256, 0, s>>>(o, n0, n1, n2, num);
  const long long tiles = (n + 255) / 256;
  const unsigned blocks = (unsigned)std::min<long long>(tiles, kVolumeBlocks);
  const long long chunk = (tiles + blocks - 1) / blocks * 256;
  branch_volume_kernel<<<blocks, 256, 0, s>>>(parsing, n0, n1, n2, num, chunk, o);
  const int skew = (int)(reinterpret_cast<uintptr_t>(skeleton) & 15);
  branch_skeleton_kernel<<<grid_for((n + skew + 15) / 16), 256, 0, s>>>(parsing, skeleton, sqdist, n0, n1, n2, num, skew, o);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// ---- wall distance pass ---------------------------------------------------------------------------------------
// Per label, over its skeleton voxels that have a feature in `indices` (the feature transform of the EDT with spacing): their
// count, the exact sums of the squared index offsets per axis, and the minimum / maximum of the squared physical distance
// (dt_0^2 + dt_1^2) + dt_2^2 with dt_a = (double)(index_a - coordinate_a) * s_a, each product and sum rounded on its own as numpy
// does.  Integer sums, and minima / maxima of non-negative doubles through their bit patterns (br_maxf_kernel of edt.hip): no order
// of execution shows in a result.

__global__ void __launch_bounds__(256)
branch_wall_init_kernel(BranchWallOut o, int num) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k == 0) *o.status = 0;
  if (k > num) return;
  o.wall_count[k] = 0;
  for (int a = 0; a < 3; ++a) o.offset_sq_sum[3 * k + a] = 0;
  o.wall_sq_min[k] = __builtin_huge_val();
  o.wall_sq_max[k] = 0.0;
}

struct WallTables { u64 *count, *sq_sum, *sq_min, *sq_max; };

// One voxel per lane, i valid where `set`; called by whole waves.  A label outside 0 .. num sets the status and is ignored.
__device__ __forceinline__ void wall_step(const int* __restrict__ parsing, const int* __restrict__ indices, long long n, int n1, int n2,
                                          int num, double s0, double s1, double s2, long long i, bool set, const WallTables& t,
                                          int* __restrict__ status) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  int a = 0;
  u64 q[3] = {0ull, 0ull, 0ull};
  u64 bits = 0;                                          // the squared distance as its bit pattern
  if (set) {
    a = parsing[i];
    if (a < 0 || a > num) { *status = 1; a = 0; }
    const int j0 = a > 0 ? indices[i] : -1;
    if (j0 < 0) a = 0;                                   // a voxel without a feature is not measured
    else {
      const Vox3 p = vox3(i, n1, n2);
      const int d0 = j0 - p.i0, d1 = indices[i + n] - p.i1, d2 = indices[i + 2 * n] - p.i2;
      q[0] = (u64)((long long)d0 * d0);
      q[1] = (u64)((long long)d1 * d1);
      q[2] = (u64)((long long)d2 * d2);
      const double t0 = (double)d0 * s0, t1 = (double)d1 * s1, t2 = (double)d2 * s2;
      bits = __builtin_bit_cast(u64, (t0 * t0 + t1 * t1) + t2 * t2);
    }
  }
  // wave-uniform from here: one label of the wave at a time, reduced over the lanes that hold it
  u64 pending = __ballot(a > 0);
  while (pending) {
    const int first = __builtin_ctzll(pending);
    const int label = dpp_settle(__shfl(a, first, 64));
    const bool mine = a == label;
    const u64 holders = __ballot(mine);
    u64 sum[3], lo = mine ? bits : ~0ull, hi = mine ? bits : 0ull;
#pragma unroll
    for (int k = 0; k < 3; ++k) sum[k] = mine ? q[k] : 0ull;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) sum[k] += shfl_xor_settled(sum[k], off);
      lo = std::min(lo, shfl_xor_settled(lo, off));
      hi = std::max(hi, shfl_xor_settled(hi, off));
    }
    if (lane == first) {
      atomicAdd(&t.count[label], lanes(holders));
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (sum[k]) atomicAdd(&t.sq_sum[3 * label + k], sum[k]);
      if (t.sq_min[label] > lo) atomicMin(&t.sq_min[label], lo);
      if (t.sq_max[label] < hi) atomicMax(&t.sq_max[label], hi);
    }
    pending &= ~holders;
  }
}

// the skeleton stream of branch_skeleton_kernel: 16 bytes per lane from 16-byte aligned addresses, `parsing` and `indices` at set
// voxels only
__global__ void __launch_bounds__(256)
branch_wall_kernel(const int* __restrict__ parsing, const unsigned char* __restrict__ skel, const int* __restrict__ indices, int n0,
                   int n1, int n2, int num, double s0, double s1, double s2, int skew, BranchWallOut o) {
  const long long n = (long long)n0 * n1 * n2, stream = n + skew;
  const unsigned char* const aligned = skel - skew;
  const WallTables t{reinterpret_cast<u64*>(o.wall_count), reinterpret_cast<u64*>(o.offset_sq_sum), reinterpret_cast<u64*>(o.wall_sq_min),
                     reinterpret_cast<u64*>(o.wall_sq_max)};
  for (long long base = blockIdx.x * 4096ll; base < stream; base += (long long)gridDim.x * 4096) {
    const long long at = base + 16ll * threadIdx.x;
    u64 half[2] = {0ull, 0ull};
    if (at >= skew && at + 16 <= stream) {
      const uint4 w = *reinterpret_cast<const uint4*>(aligned + at);
      half[0] = (u64)w.y << 32 | w.x;
      half[1] = (u64)w.w << 32 | w.z;
    } else {                                             // the ends of the volume: byte by byte, nothing outside it is read
      for (int b = 0; b < 16; ++b)
        if (at + b >= skew && at + b < stream) half[b >> 3] |= (u64)aligned[at + b] << (8 * (b & 7));
    }
    if (__ballot((half[0] | half[1]) != 0) == 0) continue;   // (wave-uniform)
#pragma unroll 1
    for (int b = 0; b < 16; ++b) {
      const bool set = ((b < 8 ? half[0] : half[1]) >> (8 * (b & 7)) & 0xffull) != 0;
      if (__ballot(set) == 0) continue;                  // (wave-uniform)
      wall_step(parsing, indices, n, n1, n2, num, s0, s1, s2, at + b - skew, set, t, o.status);
    }
  }
}

int launch_branch_wall_stats(const int* parsing, const unsigned char* skeleton, const int* indices, int n0, int n1, int n2, int num,
                             double s0, double s1, double s2, BranchWallOut o, hipStream_t s) {
  SEUNET_CHECK(parsing && skeleton && indices && o.wall_count && o.offset_sq_sum && o.wall_sq_min && o.wall_sq_max && o.status,
               "branch_wall_stats: null argument");
  if (volume_check("branch_wall_stats", n0, n1, n2, 0)) return 1;
  SEUNET_CHECK(num >= 0 && num <= label_stats_max_num(), "branch_wall_stats: num %d: labels 0 .. %d are supported", num,
               label_stats_max_num());
  SEUNET_CHECK(s0 > 0.0 && s1 > 0.0 && s2 > 0.0 && s0 < HUGE_VAL && s1 < HUGE_VAL && s2 < HUGE_VAL,
               "branch_wall_stats: the sampling must be three positive finite numbers, got (%g, %g, %g)", s0, s1, s2);
  const long long n = (long long)n0 * n1 * n2;
  branch_wall_init_kernel<<<blocks_256(num + 1), 256, 0, s>>>(o, num);
  const int skew = (int)(reinterpret_cast<uintptr_t>(skeleton) & 15);
  branch_wall_kernel<<<grid_for((n + skew + 15) / 16), 256, 0, s>>>(parsing, skeleton, indices, n0, n1, n2, num, s0, s1, s2, skew, o);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
