// Component labelling, the Euler number and the Betti numbers of a binary volume on the device.
//
// Reference (CPU, third-party code behind it): util.py, tree_parsing.py and atm22_skel_parse.py call skimage.measure.label /
// scipy.ndimage.label; the topological numbers are computed nowhere in it.  The definition is include/seunet_hip.h, restated in
// numpy / scipy by tests/betti_oracle.py.
//
//   union-find   components.hip's structure (labels = minimum linear index, a union is an atomicMin on the larger root, parents only
//                decrease, every link is a device-scope atomic on the true value, the final compression runs in its own launch: the
//                notes there about this chip's non-coherent caches apply unchanged), by connectivity -- links to the 3, 9 or 13
//                neighbours that precede a voxel in raster order -- on the mask or its complement, and by tile: two voxels are
//                linked only inside one tile, which includes the pre-linking of z-runs inside a wave span (a run also starts
//                where a tile starts along axis 2, wherever in a 64-voxel span that falls).  The whole volume is the one tile.
//   numbering    the roots (L[i] == i) as a packed mask, their counts per word through run_scan / scan_add (bitvol.h), and
//                label = scan[word of the root] + roots below it in the word + 1: raster order of the first voxels, no atomics.
//   table        sizes = the root counts compacted through the numbering, first = the root, boxes by integer min / max atomics.
//                Counts and boxes are grid-stride passes whose waves keep the sum / box of one component pending in registers
//                (a giant component would otherwise serialise every wave of the volume on one address).
//   cells        chi of a tile from popcounts on the packed words.  A thread holds one word of a row of CELLS: the words of the
//                2 x 2 rows (i0 - 1 .. i0, i1 - 1 .. i1) and their one-bit shifts along axis 2 give, for each of the eight subsets
//                S of the axes, the OR (closed cubes, connectivity 3) or the AND (voxels as vertices, connectivity 1) over the
//                voxels that differ along the axes of S; its popcount goes to class |S|.  Voxels outside the tile read as 0, so
//                a cell on a tile border is counted for each tile from that tile's voxels only: along axes 0 and 1 a tile of
//                length l has l + 1 cell positions of its own, along axis 2 the words are masked per tile.
//   betti        b0 = roots of the tile-cut foreground per tile; b2 = roots of the tile-cut complement at the dual connectivity
//                whose component reaches no face of its tile (fill_holes' border marking); b1 = b0 + b2 - chi, on the device.
// Integer work only: every result is independent of the order in which the device executes anything.
#include "volume.h"

namespace seunet {

namespace {

// ---- union-find by connectivity and tile ------------------------------------------------------------------------------------------
// cc_init_kernel (components.hip) with the tile cut: a run of voxels along z inside a wave span also starts where a tile starts
template <bool INVERT>
__global__ void __launch_bounds__(256)
bt_init_kernel(const unsigned char* __restrict__ vol, long long n, int Z, int p2, int* __restrict__ L) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool in = i < n;
  const bool fg = in && ((vol[in ? i : 0] != 0) != INVERT);
  const bool cut = in && ((int)(i % Z) % p2) == 0;           // a row starts, or a tile starts inside the row
  const u64 m = __ballot(fg), c = __ballot(cut);
  const u64 starts = m & (~(m << 1) | c | 1ull);
  if (!in) return;
  if (!fg) { L[i] = -1; return; }
  const u64 below = starts & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));
  const int s = 63 - __builtin_clzll(below);
  L[i] = (int)(i - lane + s);
}

// Links to the raster-preceding neighbours with at most CONN differing coordinates: 3, 9 or 13 of them.  A neighbour is taken only
// inside the voxel's tile; the faces of the volume are tile faces, so this is the bounds test as well.
template <int CONN>
__global__ void __launch_bounds__(256)
bt_merge_kernel(int* L, long long n, int H, int W, int Z, TileCut t) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  if (L[i] < 0) return;
  const int z = (int)(i % Z);
  const long long r = i / Z;
  const int y = (int)(r % W), x = (int)(r / W);
  const bool lo0 = x % t.p0 == 0;
  const bool lo1 = y % t.p1 == 0, hi1 = (y + 1) % t.p1 == 0 || y == W - 1;
  const bool lo2 = z % t.p2 == 0, hi2 = (z + 1) % t.p2 == 0 || z == Z - 1;
#pragma unroll
  for (int dx = -1; dx <= 0; ++dx)
#pragma unroll
    for (int dy = -1; dy <= (dx < 0 ? 1 : 0); ++dy)
#pragma unroll
      for (int dz = -1; dz <= ((dx < 0 || dy < 0) ? 1 : -1); ++dz) {
        if ((dx != 0) + (dy != 0) + (dz != 0) > CONN) continue;
        if ((dx < 0 && lo0) || (dy < 0 && lo1) || (dy > 0 && hi1) || (dz < 0 && lo2) || (dz > 0 && hi2)) continue;
        // (0, 0, -1): already linked inside a wave span by bt_init_kernel, except across the span boundary
        if (dx == 0 && dy == 0 && (i & 63) != 0) continue;
        const long long j = i + ((long long)dx * W + dy) * Z + dz;
        if (L[j] >= 0) cc_union(L, (int)i, (int)j);
      }
}

// raster index of the tile of voxel (x, y, z)
__device__ __forceinline__ int tile_of(const TileCut& t, int x, int y, int z) { return ((x / t.p0) * t.t1 + y / t.p1) * t.t2 + z / t.p2; }

// Workgroups of the grid-stride passes below: 8192 waves, about what the chip holds.  Their waves keep a pending (destination,
// sum) pair in registers over the chunks they visit and add it when the destination changes: a volume whose voxels nearly all share
// one destination -- one tile, one giant component -- costs thousands of atomics on that address instead of one per wave.
constexpr int kStrideBlocks = 2048;
static inline unsigned stride_blocks(long long items) { return (unsigned)std::min<long long>((items + 255) / 256, kStrideBlocks); }

// table[3 tile + col] += the roots of the tile (flag: only those whose flag is 0).  A wave whose roots share a tile adds them to its
// pending pair; a wave whose roots lie in several tiles adds one by one.
__global__ void __launch_bounds__(256)
bt_roots_kernel(const int* __restrict__ L, const unsigned char* __restrict__ flag, long long n, int W, int Z, TileCut t,
                int* __restrict__ table, int col) {
  const int lane = threadIdx.x & 63;
  int key = -1, acc = 0;                                     // wave-uniform
  for (long long base = blockIdx.x * 256ll; base < n; base += gridDim.x * 256ll) {
    const long long i = base + threadIdx.x;
    const bool root = i < n && L[i] == (int)i && (!flag || flag[i] == 0);
    const u64 roots = __ballot(root);
    if (!roots) continue;                                    // wave-uniform
    int tile = -1;
    if (root) {
      const Vox3 p = vox3(i, W, Z);
      tile = tile_of(t, p.i0, p.i1, p.i2);
    }
    const int lead_tile = dpp_settle(__shfl(tile, __builtin_ctzll(roots), 64));
    if (__ballot(root && tile == lead_tile) == roots) {
      if (lead_tile != key) {
        if (lane == 0 && acc) atomicAdd(&table[3ll * key + col], acc);
        key = lead_tile;
        acc = 0;
      }
      acc += (int)__popcll(roots);
    } else if (root) {
      atomicAdd(&table[3ll * tile + col], 1);
    }
  }
  if (lane == 0 && acc) atomicAdd(&table[3ll * key + col], acc);
}

// components of the complement that reach a face of their tile (cc_border_kernel of components.hip, by tile)
__global__ void __launch_bounds__(256)
bt_border_kernel(const int* __restrict__ L, long long n, int H, int W, int Z, TileCut t, unsigned char* __restrict__ flag) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const int r = L[i];
  if (r < 0) return;
  const Vox3 p = vox3(i, W, Z);
  const int x = p.i0, y = p.i1, z = p.i2;
  const bool face = x % t.p0 == 0 || (x + 1) % t.p0 == 0 || x == H - 1 || y % t.p1 == 0 || (y + 1) % t.p1 == 0 || y == W - 1 ||
                    z % t.p2 == 0 || (z + 1) % t.p2 == 0 || z == Z - 1;
  if (face) flag[r] = 1;
}

template <bool INVERT>
void union_find(const unsigned char* vol, int H, int W, int Z, int conn, const TileCut& t, int* L, hipStream_t s) {
  const long long n = (long long)H * W * Z;
  const unsigned blocks = blocks_256(n);
  bt_init_kernel<INVERT><<<blocks, 256, 0, s>>>(vol, n, Z, t.p2, L);
  if (conn == 1) bt_merge_kernel<1><<<blocks, 256, 0, s>>>(L, n, H, W, Z, t);
  else if (conn == 2) bt_merge_kernel<2><<<blocks, 256, 0, s>>>(L, n, H, W, Z, t);
  else bt_merge_kernel<3><<<blocks, 256, 0, s>>>(L, n, H, W, Z, t);
  launch_cc_compress(L, n, s);
}

// ---- dense numbering ------------------------------------------------------------------------------------------------------------------
// the packed mask of the roots and its counts per word: one wave per word, as pack_bits
__global__ void __launch_bounds__(256)
bt_root_bits_kernel(const int* __restrict__ L, BitGeom g, u64* __restrict__ roots, unsigned* __restrict__ cnt) {
  const long long t = (blockIdx.x * 256ll + threadIdx.x) >> 6;      // wave-uniform
  if (t >= g.words) return;
  const int lane = threadIdx.x & 63;
  const int k = (int)(t % g.W) * 64 + lane;
  const long long v = (t / g.W) * g.n2 + k;
  const u64 m = __ballot(k < g.n2 && L[k < g.n2 ? v : 0] == (int)v);
  if (lane == 0) {
    roots[t] = m;
    cnt[t] = (unsigned)__popcll(m);
  }
}

// number of the component with root r: the roots before it in raster order, plus one
__device__ __forceinline__ int number_of(int r, const BitGeom& g, const u64* __restrict__ roots, const unsigned* __restrict__ base) {
  const int k = r % g.n2;
  const long long w = (long long)(r / g.n2) * g.W + (k >> 6);
  return (int)(base[w] + (unsigned)__popcll(roots[w] & ((1ull << (k & 63)) - 1ull))) + 1;
}

__global__ void __launch_bounds__(256)
bt_number_kernel(const int* __restrict__ L, long long n, BitGeom g, const u64* __restrict__ roots, const unsigned* __restrict__ base,
                 int* __restrict__ out) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const int r = L[i];
  out[i] = r < 0 ? 0 : number_of(r, g, roots, base);
}

// ---- component table ------------------------------------------------------------------------------------------------------------------
// every root writes its component's row: size, first voxel, and the box of that voxel alone (bt_box_kernel widens it)
__global__ void __launch_bounds__(256)
bt_table_kernel(const int* __restrict__ L, const int* __restrict__ labels, const unsigned* __restrict__ counts, long long n, int W, int Z,
                long long num, long long* __restrict__ size, long long* __restrict__ first, int* __restrict__ box) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n || L[i] != (int)i) return;
  const long long k = (long long)labels[i] - 1;
  if (k < 0 || k >= num) return;                             // (cannot happen with the label call's output and count)
  const Vox3 p = vox3(i, W, Z);
  size[k] = (long long)counts[i];
  first[k] = i;
  int* b = box + 6 * k;
  b[0] = b[1] = p.i0; b[2] = b[3] = p.i1; b[4] = b[5] = p.i2;
}

// voxel count per root (cnt zeroed by the caller).  The root of a wave's first foreground voxel goes to the wave's pending pair; the
// other roots add one run of equal roots at a time (cc_count_kernel of components.hip, whose one atomic per run serialises on the
// root of a giant component).  Integer adds: the same counts.
__global__ void __launch_bounds__(256)
bt_count_kernel(const int* __restrict__ L, long long n, unsigned* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  int key = -1;                                              // wave-uniform
  unsigned acc = 0;
  for (long long base = blockIdx.x * 256ll; base < n; base += gridDim.x * 256ll) {
    const long long i = base + threadIdx.x;
    const int r = i < n ? L[i] : -1;
    const u64 fg = __ballot(r >= 0);
    if (!fg) continue;                                       // wave-uniform
    const int r0 = dpp_settle(__shfl(r, __builtin_ctzll(fg), 64));
    if (r0 != key) {
      if (lane == 0 && acc) atomicAdd(&cnt[key], acc);
      key = r0;
      acc = 0;
    }
    acc += (unsigned)__popcll(__ballot(r == r0));
    const int prev = dpp_settle(__shfl_up(r, 1, 64));
    const bool other = r >= 0 && r != r0;
    const bool lead = other && (lane == 0 || prev != r);
    const u64 leaders = __ballot(lead), oth = __ballot(other);
    if (lead) {
      const u64 after = (lane == 63) ? 0ull : ((leaders | ~oth) >> (lane + 1));
      atomicAdd(&cnt[r], (unsigned)(after ? __builtin_ctzll(after) + 1 : 64 - lane));
    }
  }
  if (lane == 0 && acc) atomicAdd(&cnt[key], acc);
}

// widen the box b = {min0, max0, min1, max1, min2, max2}.  A coherent look first: a bound only moves outwards, so one that is
// already past ours needs no atomic (most calls, once a component's box has grown).
__device__ __forceinline__ void box_update(int* b, const int (&lo)[3], const int (&hi)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (__hip_atomic_load(&b[2 * k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > lo[k]) atomicMin(&b[2 * k], lo[k]);
    if (__hip_atomic_load(&b[2 * k + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < hi[k]) atomicMax(&b[2 * k + 1], hi[k]);
  }
}

// boxes.  The label of a wave's first foreground voxel: the box of its voxels in the wave by wave minima / maxima, merged into the
// wave's pending box.  The other labels: one z-run of equal labels inside a row at a time.  Integer min / max: order-independent.
__global__ void __launch_bounds__(256)
bt_box_kernel(const int* __restrict__ labels, long long n, int W, int Z, long long num, int* __restrict__ box) {
  const int lane = threadIdx.x & 63;
  int key = 0, lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};          // wave-uniform: the pending box of label `key` (0: none)
  for (long long base = blockIdx.x * 256ll; base < n; base += gridDim.x * 256ll) {
    const long long i = base + threadIdx.x;
    int r = i < n ? labels[i] : 0;
    if (r > num) r = 0;                                      // (cannot happen with the label call's output and count)
    const u64 fg = __ballot(r > 0);
    if (!fg) continue;                                       // wave-uniform
    const int r0 = dpp_settle(__shfl(r, __builtin_ctzll(fg), 64));
    const Vox3 p = vox3(i < n ? i : 0, W, Z);
    const int c[3] = {p.i0, p.i1, p.i2};
    const bool dom = r == r0;
    int mn[3], mx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      mx[k] = wave_max(dom ? c[k] : -1);
      mn[k] = -wave_max(dom ? -c[k] : -0x7fffffff);
    }
    if (r0 != key) {
      if (lane == 0 && key > 0) box_update(box + 6ll * (key - 1), lo, hi);
      key = r0;
#pragma unroll
      for (int k = 0; k < 3; ++k) { lo[k] = mn[k]; hi[k] = mx[k]; }
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], mn[k]); hi[k] = std::max(hi[k], mx[k]); }
    }
    const int prev = dpp_settle(__shfl_up(r, 1, 64));
    const bool other = r > 0 && !dom;
    const bool lead = other && (lane == 0 || prev != r || p.i2 == 0);
    const u64 leaders = __ballot(lead), oth = __ballot(other);
    if (lead) {
      const u64 after = (lane == 63) ? 0ull : ((leaders | ~oth) >> (lane + 1));
      const int len = after ? __builtin_ctzll(after) + 1 : 64 - lane;
      const int rlo[3] = {p.i0, p.i1, p.i2}, rhi[3] = {p.i0, p.i1, p.i2 + len - 1};
      box_update(box + 6ll * (r - 1), rlo, rhi);
    }
  }
  if (lane == 0 && key > 0) box_update(box + 6ll * (key - 1), lo, hi);
}

__global__ void __launch_bounds__(256)
bt_keep_kernel(const int* __restrict__ L, const unsigned* __restrict__ counts, long long n, long long min_size,
               unsigned char* __restrict__ out) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const int r = L[i];
  out[i] = (r >= 0 && (long long)counts[r] >= min_size) ? 1 : 0;
}

// ---- cell counts ----------------------------------------------------------------------------------------------------------------------
// bits [lo, hi) of a word, clipped to the word
__device__ __forceinline__ u64 range_mask(long long lo, long long hi) {
  lo = lo < 0 ? 0 : lo;
  hi = hi > 64 ? 64 : hi;
  if (lo >= hi) return 0ull;
  const u64 m = hi - lo == 64 ? ~0ull : ((1ull << (hi - lo)) - 1ull);
  return m << lo;
}

struct CellWords { u64 x[2][2], xp[2][2]; };   // [a][b]: word w (x) and word w - 1 (xp) of row (i0 - a, i1 - b); 0 outside the tile

// the counts of one tile along axis 2 (voxels [lo2, hi2)) in cell word w: class |S| += popcount of the OR / AND over S
template <bool ALL>
__device__ __forceinline__ void cell_counts(const CellWords& c, int w, int lo2, int hi2, int (&cnt)[kCellClasses]) {
  const u64 vm = range_mask(lo2 - 64ll * w, hi2 - 64ll * w), vmp = range_mask(lo2 - 64ll * (w - 1), hi2 - 64ll * (w - 1));
  u64 v[2][2][2];                                            // [a][b][c]: c = 1 is voxel i2 - 1
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      v[a][b][0] = c.x[a][b] & vm;
      v[a][b][1] = shift_down(v[a][b][0], c.xp[a][b] & vmp);
    }
#pragma unroll
  for (int q = 0; q < kCellClasses; ++q) cnt[q] = 0;
#pragma unroll
  for (int S = 0; S < 8; ++S) {
    u64 m = v[0][0][0];
#pragma unroll
    for (int a = 0; a <= (S & 1); ++a)
#pragma unroll
      for (int b = 0; b <= ((S >> 1) & 1); ++b)
#pragma unroll
        for (int cc = 0; cc <= ((S >> 2) & 1); ++cc) m = ALL ? (m & v[a][b][cc]) : (m | v[a][b][cc]);
    cnt[(S & 1) + ((S >> 1) & 1) + ((S >> 2) & 1)] += __popcll(m);
  }
}

// One thread per word of a row of cells, grid-stride.  Along axes 0 and 1 the rows are numbered tile by tile, p + 1 positions per
// tile (the last one: its length + 1), position q of a tile using voxel row q (if q < length) and q - 1 (if q > 0) of the tile; a
// row of cells has We = n2 / 64 + 1 words, and word w is counted for every tile whose positions [lo2, hi2] meet it.  A thread keeps
// the counts of one tile pending and adds them when its tile changes; at the end a workgroup whose threads all hold one tile (the
// whole volume as one tile: every workgroup) adds once per class, else a wave that does, else every thread.  Integer atomics on
// the tile's counters in every case.
template <bool ALL>
__global__ void __launch_bounds__(256)
bt_cells_kernel(const u64* __restrict__ bits, BitGeom g, TileCut t, int We, long long items, u64* __restrict__ cells) {
  __shared__ int s_tile;
  __shared__ int s_part[4][kCellClasses];
  const int lane = threadIdx.x & 63;
  int key = -1, acc[kCellClasses] = {0, 0, 0, 0};            // per thread
  for (long long idx = blockIdx.x * 256ll + threadIdx.x; idx < items; idx += gridDim.x * 256ll) {
    CellWords c;
    const int w = (int)(idx % We);
    const long long r = idx / We;
    const int E1 = g.n1 + t.t1;
    const int e1 = (int)(r % E1), e0 = (int)(r / E1);
    const int T0 = e0 / (t.p0 + 1), q0 = e0 % (t.p0 + 1), T1 = e1 / (t.p1 + 1), q1 = e1 % (t.p1 + 1);
    const int len0 = std::min(t.p0, g.n0 - T0 * t.p0), len1 = std::min(t.p1, g.n1 - T1 * t.p1);
    const int T01 = (T0 * t.t1 + T1) * t.t2;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const bool ok = (a ? q0 > 0 : q0 < len0) && (b ? q1 > 0 : q1 < len1);
        const long long row = (long long)(T0 * t.p0 + q0 - a) * g.n1 + (T1 * t.p1 + q1 - b);
        c.x[a][b] = ok && w < g.W ? bits[row * g.W + w] : 0ull;
        c.xp[a][b] = ok && w > 0 ? bits[row * g.W + w - 1] : 0ull;
      }
    const int T2a = w == 0 ? 0 : (64 * w - 1) / t.p2, T2b = std::min(t.t2 - 1, (64 * w + 63) / t.p2);
    for (int T2 = T2a; T2 <= T2b; ++T2) {
      int cnt[kCellClasses];
      cell_counts<ALL>(c, w, T2 * t.p2, std::min(T2 * t.p2 + t.p2, g.n2), cnt);
      if (T01 + T2 != key) {
        if (key >= 0)
#pragma unroll
          for (int q = 0; q < kCellClasses; ++q)
            if (acc[q]) atomicAdd(&cells[(long long)key * kCellClasses + q], (u64)acc[q]);
        key = T01 + T2;
#pragma unroll
        for (int q = 0; q < kCellClasses; ++q) acc[q] = 0;
      }
#pragma unroll
      for (int q = 0; q < kCellClasses; ++q) acc[q] += cnt[q];
    }
  }
  // (thread 0 of a workgroup, and lane 0 of a wave, has an item wherever one of its threads has: its key is a tile then)
  if (threadIdx.x == 0) s_tile = key;
  __syncthreads();
  const int blk_tile = s_tile;
  if (blk_tile >= 0 && __syncthreads_and(key == blk_tile || key < 0)) {
#pragma unroll
    for (int q = 0; q < kCellClasses; ++q) {
      const int sum = wave_sum(acc[q]);
      if (lane == 0) s_part[threadIdx.x >> 6][q] = sum;
    }
    __syncthreads();
    if (threadIdx.x < kCellClasses) {
      const int q = threadIdx.x, sum = s_part[0][q] + s_part[1][q] + s_part[2][q] + s_part[3][q];
      if (sum) atomicAdd(&cells[(long long)blk_tile * kCellClasses + q], (u64)sum);
    }
    return;
  }
  const int lead = dpp_settle(__shfl(key, 0, 64));
  if (lead >= 0 && __all(key == lead || key < 0)) {
#pragma unroll
    for (int q = 0; q < kCellClasses; ++q) {
      const int sum = wave_sum(acc[q]);
      if (lane == 0 && sum) atomicAdd(&cells[(long long)lead * kCellClasses + q], (u64)sum);
    }
    return;
  }
  if (key >= 0)
#pragma unroll
    for (int q = 0; q < kCellClasses; ++q)
      if (acc[q]) atomicAdd(&cells[(long long)key * kCellClasses + q], (u64)acc[q]);
}

// chi per tile from its cell counts, and b1 = b0 + b2 - chi into the table
__global__ void __launch_bounds__(256)
bt_finish_kernel(const u64* __restrict__ cells, long long tiles, int conn, long long* __restrict__ chi_out, int* __restrict__ table) {
  const long long T = blockIdx.x * 256ll + threadIdx.x;
  if (T >= tiles) return;
  const u64* c = cells + T * kCellClasses;
  // connectivity 3: class 0 = cubes, 1 = faces, 2 = edges, 3 = vertices; connectivity 1: 0 = voxels, 1 = pairs, 2 = squares, 3 = cubes
  const long long alt = (long long)c[0] - (long long)c[1] + (long long)c[2] - (long long)c[3];
  const long long chi = conn == 3 ? -alt : alt;
  if (chi_out) chi_out[T] = chi;
  if (table) table[3 * T + 1] = table[3 * T] + table[3 * T + 2] - (int)chi;
}

int run_euler(const unsigned char* vol, int n0, int n1, int n2, const TileCut& t, int conn, const EulerWs& w, long long* chi_dev,
              int* table, hipStream_t s) {
  const BitGeom g = bit_geom(n0, n1, n2);
  const long long tiles = t.tiles();
  const int We = n2 / 64 + 1;
  const long long items = (long long)(n0 + t.t0) * (n1 + t.t1) * We;
  pack_bits(vol, nullptr, g, w.bits, nullptr, s);
  SEUNET_HIP(hipMemsetAsync(w.cells, 0, (size_t)tiles * kCellClasses * sizeof(u64), s));
  if (conn == 3) bt_cells_kernel<false><<<stride_blocks(items), 256, 0, s>>>(w.bits, g, t, We, items, w.cells);
  else bt_cells_kernel<true><<<stride_blocks(items), 256, 0, s>>>(w.bits, g, t, We, items, w.cells);
  bt_finish_kernel<<<blocks_256(tiles), 256, 0, s>>>(w.cells, tiles, conn, chi_dev, table);
  return 0;
}

int check_args(const char* what, int n0, int n1, int n2, int conn, bool dual) {
  if (volume_check(what, n0, n1, n2, 0)) return 1;
  if (dual) SEUNET_CHECK(conn == 1 || conn == 3, "%s: connectivity %d: 1 (6 neighbours) or 3 (26 neighbours); 18 neighbours have no dual", what, conn);
  else SEUNET_CHECK(conn >= 1 && conn <= 3, "%s: connectivity %d: 1, 2 or 3 (6, 18 or 26 neighbours)", what, conn);
  return 0;
}

}  // namespace

size_t label_workspace_bytes(int n0, int n1, int n2) { return measured(label_ws, n0, n1, n2); }
size_t euler_workspace_bytes(int n0, int n1, int n2, TileCut t) {
  WsCarver c(nullptr);
  euler_ws(c, n0, n1, n2, t.tiles());
  return c.bytes();
}
size_t betti_workspace_bytes(int n0, int n1, int n2, TileCut t) {
  WsCarver c(nullptr);
  betti_ws(c, n0, n1, n2, t.tiles());
  return c.bytes();
}

int launch_label(const unsigned char* vol, int n0, int n1, int n2, int conn, int* labels_out, int* num_dev, void* workspace,
                 size_t ws_bytes, hipStream_t s) {
  if (check_args("label", n0, n1, n2, conn, false)) return 1;
  SEUNET_CHECK(vol && labels_out && workspace, "label: null argument");
  WsCarver carve(workspace);
  const LabelWs w = label_ws(carve, n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "label: workspace too small");
  const long long n = (long long)n0 * n1 * n2;
  const BitGeom g = bit_geom(n0, n1, n2);
  union_find<false>(vol, n0, n1, n2, conn, tile_cut(n0, n1, n2, n0, n1, n2), w.labels, s);
  bt_root_bits_kernel<<<(unsigned)((g.words + 3) / 4), 256, 0, s>>>(w.labels, g, w.roots, w.cnt);
  if (run_scan(w.cnt, nullptr, g.words, w.blk, nullptr, w.total, s)) return 1;
  scan_add(w.cnt, w.blk, g.words, w.total, w.base, s);
  bt_number_kernel<<<blocks_256(n), 256, 0, s>>>(w.labels, n, g, w.roots, w.base, labels_out);
  if (num_dev) SEUNET_HIP(hipMemcpyAsync(num_dev, w.base + g.words, sizeof(int), hipMemcpyDeviceToDevice, s));
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_component_table(const int* labels, int n0, int n1, int n2, long long num, long long* size, long long* first, int* box,
                           void* workspace, size_t ws_bytes, hipStream_t s) {
  if (volume_check("component_table", n0, n1, n2, 0)) return 1;
  const long long n = (long long)n0 * n1 * n2;
  SEUNET_CHECK(labels && size && first && box && workspace, "component_table: null argument");
  SEUNET_CHECK(num >= 1 && num <= n, "component_table: %lld components in %lld voxels", num, n);
  WsCarver carve(workspace);
  const LabelWs w = label_ws(carve, n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "component_table: workspace too small");
  SEUNET_HIP(hipMemsetAsync(w.counts, 0, (size_t)n * 4, s));
  bt_count_kernel<<<stride_blocks(n), 256, 0, s>>>(w.labels, n, w.counts);
  bt_table_kernel<<<blocks_256(n), 256, 0, s>>>(w.labels, labels, w.counts, n, n1, n2, num, size, first, box);
  bt_box_kernel<<<stride_blocks(n), 256, 0, s>>>(labels, n, n1, n2, num, box);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_remove_small(const unsigned char* vol, int n0, int n1, int n2, long long min_size, int conn, unsigned char* out,
                        void* workspace, size_t ws_bytes, hipStream_t s) {
  if (check_args("remove_small_objects", n0, n1, n2, conn, false)) return 1;
  SEUNET_CHECK(vol && out && workspace, "remove_small_objects: null argument");
  WsCarver carve(workspace);
  const CcWs w = cc_ws(carve, n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "remove_small_objects: workspace too small");
  const long long n = (long long)n0 * n1 * n2;
  SEUNET_HIP(hipMemsetAsync(w.counts, 0, (size_t)n * 4, s));
  union_find<false>(vol, n0, n1, n2, conn, tile_cut(n0, n1, n2, n0, n1, n2), w.labels, s);
  bt_count_kernel<<<stride_blocks(n), 256, 0, s>>>(w.labels, n, w.counts);
  bt_keep_kernel<<<blocks_256(n), 256, 0, s>>>(w.labels, w.counts, n, min_size, out);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_euler(const unsigned char* vol, int n0, int n1, int n2, TileCut t, int conn, long long* chi_dev, void* workspace,
                 size_t ws_bytes, hipStream_t s) {
  if (check_args("euler", n0, n1, n2, conn, true)) return 1;
  SEUNET_CHECK(vol && chi_dev && workspace, "euler: null argument");
  WsCarver carve(workspace);
  const EulerWs w = euler_ws(carve, n0, n1, n2, t.tiles());
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "euler: workspace too small");
  if (run_euler(vol, n0, n1, n2, t, conn, w, chi_dev, nullptr, s)) return 1;
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_betti(const unsigned char* vol, int n0, int n1, int n2, TileCut t, int conn, int* table_dev, void* workspace, size_t ws_bytes,
                 hipStream_t s) {
  if (check_args("betti", n0, n1, n2, conn, true)) return 1;
  SEUNET_CHECK(vol && table_dev && workspace, "betti: null argument");
  WsCarver carve(workspace);
  const BettiWs w = betti_ws(carve, n0, n1, n2, t.tiles());
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "betti: workspace too small");
  const long long n = (long long)n0 * n1 * n2;
  const unsigned blocks = blocks_256(n);
  SEUNET_HIP(hipMemsetAsync(table_dev, 0, (size_t)t.tiles() * 3 * sizeof(int), s));
  SEUNET_HIP(hipMemsetAsync(w.flag, 0, (size_t)n, s));
  union_find<false>(vol, n0, n1, n2, conn, t, w.labels, s);
  bt_roots_kernel<<<stride_blocks(n), 256, 0, s>>>(w.labels, nullptr, n, n1, n2, t, table_dev, 0);
  union_find<true>(vol, n0, n1, n2, 4 - conn, t, w.labels, s);          // the dual: 3 <-> 1
  bt_border_kernel<<<blocks, 256, 0, s>>>(w.labels, n, n0, n1, n2, t, w.flag);
  bt_roots_kernel<<<stride_blocks(n), 256, 0, s>>>(w.labels, w.flag, n, n1, n2, t, table_dev, 2);
  if (run_euler(vol, n0, n1, n2, t, conn, w.euler, nullptr, table_dev, s)) return 1;
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
