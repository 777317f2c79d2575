// Labelled surface meshing on the device: an int32 label volume with values 0 .. num to the meshes of all
// its labels at once, concatenated in label order.
//
// Reference (CPU): ours_skel_parse.py:1101-1152 (Topology_Tree.sub_model) and tree_parsing.py:167-196 call
// marching_cubes(tree_parsing == k, 0.95) for every k -- num full-volume extractions.  Here the mesh of label k is by definition
// mesh.hip's marching_cubes(L == k) (tests/mesh_oracle.py): same positions, same numbering, same orientation; the
// result is the concatenation over k = 1 .. num (tests/mesh_label_oracle.py), and every byte equals that oracle.
//
// One wavefront works on one 64-voxel word of a row (the word grid of bitvol.h), one lane per voxel / cell, as in mesh.hip, but on
// the labels themselves:
//   count  a lane reads the 8 corners of its cell.  Its voxel owns, per axis with a +1 neighbour of another label, one vertex
//          item for each of the two labels that is not 0 (low-end label first): at most 3 x 2 = 6.  Its cell owns, for every
//          distinct non-zero label among the corners, the table's triangles of the configuration "corner == label": at most 8
//          over all set partitions of the corners (tests/test_mesh_label_host.py walks them).  So 3 ballots rank the vertex
//          items of a word and 4 the triangle items.  A word whose 2 x 2 rows x 65 voxels carry one value leaves after its loads
//          and is marked, so that the two later passes over the words leave it after one byte.
//          Items per label are summed over the wavefront and added with one integer atomic per distinct label (a count does
//          not depend on the order of its additions; no atomic ever hands out a position).
//   scan   run_scan (bitvol.h) over the per-word counts (item numbering in raster order) and over the per-label counts
//          (vert_ptr / face_ptr).  The host reads V, F, the largest label and the status once.
//   keys   the label of every item, in raster order.
//   sort   stable LSD radix sort of (label, raster index), 8-bit digits, one pass for num < 256 and two otherwise: per-block
//          digit counts, run_scan over them digit-major, then a rank inside the block that no atomic takes part in -- lanes in
//          item order, the lanes of one digit found with 8 ballots, one sub-histogram per wave advanced round by round and
//          summed over the earlier waves.  The last pass writes the inverse permutation perm[raster index] = position.
//   emit   every vertex goes to verts[perm[item]]; every triangle to faces[fperm[item]], its corners through perm once.
// This file is compiled with -ffp-contract=off like mesh.hip: the one float32 addition per vertex is a single rounded operation.
#include "volume.h"
#include "mesh_table.h"

namespace seunet {

namespace {

__constant__ MeshTable kLabelTable = make_mesh_table();

struct LabelGeom : BitGeom {  // the word grid of the label volume's rows: no packed volume is stored, the lanes read the labels
  int limit;                  // the largest label accepted: num, or kMeshLabelMax when the call finds num itself
  int cells;                  // 0: an extent of 1, no cell and by definition no vertex either
};

// a label outside 0 .. limit is reported by the count pass and is background everywhere: no index is ever formed from it
__device__ __forceinline__ int clean_label(int v, int limit) { return (unsigned)v <= (unsigned)limit ? v : 0; }

// What a lane knows about its voxel (i, j, k) and the cell above it.  c[4 d0 + 2 d1 + d2] = label at (i + d0, j + d1, k + d2);
// a corner that does not exist, and every corner of a lane past the row's end, repeats c[0], so it makes no vertex.
struct Lane {
  int c[8];
  int i, j, k;
  bool has0, has1, has2;      // the voxel has a +1 neighbour along the axis
  bool cell;                  // all eight corners exist
  int raw;                    // the voxel's label as stored (the word's first voxel for a lane past the row's end)
};

__device__ __forceinline__ Lane load_lane(const int* __restrict__ L, const LabelGeom& g, long long t, int lane) {
  Lane a;
  const int w = (int)(t % g.W);
  const long long row = t / g.W;
  a.j = (int)(row % g.n1); a.i = (int)(row / g.n1); a.k = 64 * w + lane;
  const bool in = a.k < g.n2;
  a.has0 = in && a.i + 1 < g.n0;
  a.has1 = in && a.j + 1 < g.n1;
  a.has2 = a.k + 1 < g.n2;
  a.cell = a.has0 && a.has1 && a.has2;
  const long long d0 = (long long)g.n1 * g.n2, d1 = g.n2;
  const long long at = row * g.n2 + (in ? a.k : 64 * w);      // 64 w < n2: the word exists
  a.raw = L[at];
  const int p = clean_label(a.raw, g.limit);
  a.c[0] = p;
  a.c[1] = a.has2 ? clean_label(L[at + 1], g.limit) : p;
  a.c[2] = a.has1 ? clean_label(L[at + d1], g.limit) : p;
  a.c[4] = a.has0 ? clean_label(L[at + d0], g.limit) : p;
  a.c[3] = a.cell ? clean_label(L[at + d1 + 1], g.limit) : p;
  a.c[5] = a.cell ? clean_label(L[at + d0 + 1], g.limit) : p;
  a.c[6] = a.cell ? clean_label(L[at + d0 + d1], g.limit) : p;
  a.c[7] = a.cell ? clean_label(L[at + d0 + d1 + 1], g.limit) : p;
  return a;
}

// all 8 corners of all 64 lanes carry one value: no vertex item, no triangle item (wave-uniform answer)
__device__ __forceinline__ bool wave_flat(const Lane& a) {
  const int v = __builtin_amdgcn_readfirstlane(a.c[0]);
  bool differs = false;
#pragma unroll
  for (int q = 0; q < 8; ++q) differs = differs || a.c[q] != v;
  return __ballot(differs) == 0ull;
}

// the +1 neighbour's label along axis 0 / 1 / 2 (= the voxel's own where there is none)
__device__ __forceinline__ int neighbour(const Lane& a, int axis) { return axis == 0 ? a.c[4] : (axis == 1 ? a.c[2] : a.c[1]); }

// vertex items of the lane's voxel: per axis, low-end label then high-end label, zero labels left out.  At most 6.
__device__ __forceinline__ int lane_vertices(const Lane& a) {
  int n = 0;
#pragma unroll
  for (int axis = 0; axis < 3; ++axis) {
    const int q = neighbour(a, axis);
    if (q != a.c[0]) n += (a.c[0] != 0) + (q != 0);
  }
  return n;
}

__device__ __forceinline__ int corner(const Lane& a, int s) {
  int v = a.c[0];
#pragma unroll
  for (int r = 1; r < 8; ++r) v = s == r ? a.c[r] : v;
  return v;
}

// f(label, configuration) for every distinct non-zero label among the corners of the lane's cell, in order of first corner
template <typename F> __device__ __forceinline__ void for_each_cell_label(const Lane& a, F f) {
  if (!a.cell) return;
#pragma unroll 1
  for (int s = 0; s < 8; ++s) {
    const int l = corner(a, s);
    if (l == 0) continue;
    int cfg = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) cfg |= (a.c[r] == l ? 1 : 0) << r;
    if (cfg & ((1 << s) - 1)) continue;                        // an earlier corner carries this label
    f(l, cfg);
  }
}

// triangle items of the lane's cell: at most 8 (see the head of the file)
__device__ __forceinline__ int lane_triangles(const Lane& a) {
  int n = 0;
  for_each_cell_label(a, [&](int, int cfg) { n += kLabelTable.count[cfg]; });
  return n;
}

// hist[label] += n over the wavefront, one atomic per distinct label: a branch's surface puts most of a word's items on one label,
// and a single word of memory takes atomics far more slowly than the waves produce them.  n <= 8.  Called by all 64 lanes.
__device__ __forceinline__ void wave_add(unsigned* __restrict__ hist, int lane, int label, unsigned n) {
  u64 pending = __ballot(n != 0u);
  while (pending != 0ull) {                                    // uniform: one round per distinct label
    const int leader = __ffsll((long long)pending) - 1;
    const int lab = __shfl(label, leader, 64);
    const bool same = n != 0u && label == lab;
    const unsigned total = (unsigned)ballot_sum<4>(same ? (int)n : 0);
    if (lane == leader) atomicAdd(&hist[lab], total);
    pending &= ~__ballot(same);
  }
}

__global__ void __launch_bounds__(256)
label_count_kernel(const int* __restrict__ L, LabelGeom g, MeshLabelWs w) {
  const long long t = (blockIdx.x * 256ll + threadIdx.x) >> 6;
  if (t >= g.words) return;                                    // whole wavefronts leave together
  const int lane = threadIdx.x & 63;
  const Lane a = load_lane(L, g, t, lane);
  const bool flat = wave_flat(a) || !g.cells;
  // every voxel is the c[0] of exactly one lane: the label check and the largest label ride on the loads
  const u64 negative = __ballot(a.raw < 0), large = __ballot(a.raw > g.limit);
  const int top = flat && g.cells ? a.c[0] : wave_max(a.c[0]);
  unsigned nv = 0u, nf = 0u;
  BitPlanes<3> vb = {};
  if (!flat) {                                                 // uniform; most words of a CT carry one value
    const int mv = lane_vertices(a), mf = lane_triangles(a);
    vb = ballot_planes<3>(mv);
    nv = (unsigned)plane_sum(vb);
    nf = (unsigned)ballot_sum<4>(mf);
    // items per label.  Labels are clean: 0 .. limit <= kMeshLabelMax, inside the two arrays.  Every call below is made by the
    // whole wavefront (n = 0: nothing to add).
    const int p = a.c[0];
    unsigned mine = 0u;
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
      const int q = neighbour(a, axis);
      mine += q != p && p != 0;
      wave_add(w.vhist, lane, q, q != p && q != 0 ? 1u : 0u);
    }
    wave_add(w.vhist, lane, p, mine);
#pragma unroll 1
    for (int s = 0; s < 8; ++s) {                              // the walk of for_each_cell_label, in step for the whole wavefront
      const int l = a.cell ? corner(a, s) : 0;
      int cfg = 0;
#pragma unroll
      for (int r = 0; r < 8; ++r) cfg |= (a.c[r] == l ? 1 : 0) << r;
      const bool first = l != 0 && (cfg & ((1 << s) - 1)) == 0;
      wave_add(w.fhist, lane, l, first ? (unsigned)kLabelTable.count[cfg] : 0u);
    }
  }
  if (lane == 0) {
    w.vb0[t] = vb.b[0]; w.vb1[t] = vb.b[1]; w.vb2[t] = vb.b[2];
    w.vcnt[t] = nv;
    w.fcnt[t] = nf;
    w.active[t] = flat ? 0 : 1;
    if (negative) atomicOr(&w.rec->status, 1);
    if (large) atomicOr(&w.rec->status, 2);
    // the plain read can only be stale towards smaller values: then the atomic is issued once more than needed
    if (top > __hip_atomic_load(&w.rec->max_label, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&w.rec->max_label, top);
  }
}

// ptr[k] = items of the labels 1 .. k = the exclusive scan at k + 1 (hist[0], the background's slot, stays 0)
__global__ void __launch_bounds__(256)
label_ptr_kernel(MeshLabelWs w, int cells, long long* __restrict__ vert_ptr, long long* __restrict__ face_ptr, int capacity) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= capacity) return;
  long long v = 0, f = 0;
  if (cells) {
    const int at = k + 1;
    v = at <= kMeshLabelMax ? (long long)w.vhist[at] + w.hvblk[at / kScanBlock] : (long long)w.htotal[0];
    f = at <= kMeshLabelMax ? (long long)w.fhist[at] + w.hfblk[at / kScanBlock] : (long long)w.htotal[1];
  }
  vert_ptr[k] = v;
  face_ptr[k] = f;
}

// ---- items in raster order: their keys, later their final places ------------------------------------------------------------------
struct ItemArgs {
  const int* labels;
  MeshLabelWs w;              // after the scans
  long long nverts, nfaces;
  // keys pass
  unsigned short *vkey, *fkey;
  // emit pass
  const unsigned *vperm, *fperm;
  float t_lo0, t_lo1;         // offset of a vertex whose low end is outside / inside its label
  float* verts;
  int* faces;
};

// raster index of the first vertex item of the voxel at bit `bit` of word tw
__device__ __forceinline__ unsigned voxel_vertex_base(const MeshLabelWs& w, long long tw, int bit) {
  const BitPlanes<3> vb = {{w.vb0[tw], w.vb1[tw], w.vb2[tw]}};
  return w.vblk[tw / kScanBlock] + w.vcnt[tw] + (unsigned)plane_sum(vb, lanes_below(bit));
}

// Raster index of the vertex item (grid edge, label): the grid edge is cube edge `edge` of the cell at (i, j, k), which exists, so
// the owning voxel and its +1 neighbours along the edge's axis and the axes before it are inside the volume.  Items of the
// owning voxel come axis by axis, the low-end label's before the high-end label's.
__device__ __forceinline__ long long edge_item(const int* __restrict__ L, const LabelGeom& g, const MeshLabelWs& w, int i, int j, int k,
                                               int edge, int label) {
  const int axis = edge >> 2, du = (edge >> 1) & 1, dv = edge & 1;
  const int o0 = i + (axis == 0 ? 0 : du), o1 = j + (axis == 0 ? du : (axis == 1 ? 0 : dv)), o2 = k + (axis == 2 ? 0 : dv);
  const long long row = (long long)o0 * g.n1 + o1, at = row * g.n2 + o2;
  const long long stride[3] = {(long long)g.n1 * g.n2, (long long)g.n2, 1ll};
  const bool has[3] = {o0 + 1 < g.n0, o1 + 1 < g.n1, o2 + 1 < g.n2};
  const int p = clean_label(L[at], g.limit);
  unsigned id = voxel_vertex_base(w, row * g.W + (o2 >> 6), o2 & 63);
#pragma unroll
  for (int b = 0; b < 2; ++b)                                   // the axes before the edge's
    if (b < axis && has[b]) {
      const int q = clean_label(L[at + stride[b]], g.limit);
      if (q != p) id += (unsigned)((p != 0) + (q != 0));
    }
  if (label != p && p != 0) ++id;                              // the high-end label's item follows the low end's
  return (long long)id;
}

template <bool KEYS> __global__ void __launch_bounds__(256) label_items_kernel(ItemArgs e, LabelGeom g) {
  const long long t = (blockIdx.x * 256ll + threadIdx.x) >> 6;
  if (t >= g.words) return;
  const int lane = threadIdx.x & 63;
  if (e.w.active[t] == 0) return;                              // uniform: the count pass found the word flat (99 % of a CT)
  const Lane a = load_lane(e.labels, g, t, lane);

  if (lane_vertices(a) != 0) {
    long long idx = (long long)voxel_vertex_base(e.w, t, lane);
    const int p = a.c[0];
    const float x[3] = {(float)a.i, (float)a.j, (float)a.k};
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
      const int q = neighbour(a, axis);
      if (q == p) continue;
#pragma unroll
      for (int high = 0; high < 2; ++high) {
        const int l = high ? q : p;
        if (l == 0) continue;
        const long long r = idx++;
        if (r >= e.nverts) continue;                            // (cannot happen with the totals of the count pass)
        if (KEYS) {
          e.vkey[r] = (unsigned short)l;
        } else {
          const long long at = e.vperm[r];
          if (at >= e.nverts) continue;                         // (a permutation of 0 .. V - 1)
          float y[3] = {x[0], x[1], x[2]};
          y[axis] = __fadd_rn(x[axis], high ? e.t_lo0 : e.t_lo1);   // label l is at the high end: its low end is outside
          float* out = e.verts + at * 3;
          out[0] = y[0]; out[1] = y[1]; out[2] = y[2];
        }
      }
    }
  }

  const int mf = lane_triangles(a);
  const BitPlanes<4> fb = ballot_planes<4>(mf);
  if ((fb.b[0] | fb.b[1] | fb.b[2] | fb.b[3]) == 0ull) return;
  long long f = (long long)(e.w.fblk[t / kScanBlock] + e.w.fcnt[t]) + plane_sum(fb, lanes_below(lane));
  for_each_cell_label(a, [&](int l, int cfg) {
    const int n = kLabelTable.count[cfg];
    for (int q = 0; q < n; ++q, ++f) {
      if (f >= e.nfaces) return;                                // (cannot happen with the totals of the count pass)
      if (KEYS) {
        e.fkey[f] = (unsigned short)l;
        continue;
      }
      const long long at = e.fperm[f];
      if (at >= e.nfaces) continue;
#pragma unroll
      for (int cn = 0; cn < 3; ++cn) {
        const long long r = edge_item(e.labels, g, e.w, a.i, a.j, a.k, kLabelTable.edges[cfg][3 * q + cn], l);
        e.faces[at * 3 + cn] = r < e.nverts ? (int)e.vperm[r] : 0;   // through the sort's inverse permutation, once
      }
    }
  });
}

// ---- stable radix sort of (label, raster index): one 8-bit digit per pass ----------------------------------------------------------
// A block owns kSortBlock consecutive items.  Counting may use atomics; the counts do not depend on their order.
__global__ void __launch_bounds__(256)
radix_hist_kernel(const unsigned short* __restrict__ key, long long n, int shift, unsigned nblocks, unsigned* __restrict__ hist) {
  __shared__ unsigned cnt[256];
  const int tid = threadIdx.x;
  cnt[tid] = 0u;
  __syncthreads();
  const long long base = blockIdx.x * (long long)kSortBlock;
#pragma unroll
  for (int r = 0; r < kSortBlock / 256; ++r) {
    const long long i = base + r * 256 + tid;
    if (i < n) atomicAdd(&cnt[(key[i] >> shift) & 255], 1u);
  }
  __syncthreads();
  hist[(size_t)tid * nblocks + blockIdx.x] = cnt[tid];         // digit-major: one scan gives every (digit, block) its base
}

// Item order inside a block: wave, then round, then lane (item = block base + 256 wave + 64 round + lane).  The rank of an item
// among the block's items of its digit = those in earlier waves + those in earlier rounds of its wave + those in lower lanes of
// its round.  Nothing here depends on which wave runs first.
__global__ void __launch_bounds__(256)
radix_scatter_kernel(const unsigned short* __restrict__ key, const unsigned* __restrict__ idx, long long n, int shift, unsigned nblocks,
                     const unsigned* __restrict__ hist, const unsigned* __restrict__ hblk, unsigned short* __restrict__ key_out,
                     unsigned* __restrict__ idx_out, unsigned* __restrict__ perm) {
  __shared__ unsigned sub[4][256];                             // per wave: items of every digit in the rounds done so far
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int q = 0; q < 4; ++q) sub[q][tid] = 0u;
  __syncthreads();
  volatile unsigned* mine = sub[wave];
  const u64 below = (1ull << lane) - 1ull;
  const long long base = blockIdx.x * (long long)kSortBlock + wave * 256;
  unsigned short k[4];
  unsigned rank[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long i = base + r * 64 + lane;
    const bool valid = i < n;
    k[r] = valid ? key[i] : (unsigned short)0;
    const unsigned d = (k[r] >> shift) & 255u;
    u64 same = __ballot(valid);                                // the valid lanes of this round with this lane's digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const u64 set = __ballot(bit);
      same &= bit ? set : ~set;
    }
    const unsigned before = mine[d];                           // the wave reads, then the first lane of each digit writes
    rank[r] = before + (unsigned)__popcll(same & below);
    if (valid && (same & below) == 0ull) mine[d] = before + (unsigned)__popcll(same);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long i = base + r * 64 + lane;
    if (i >= n) continue;
    const unsigned d = (k[r] >> shift) & 255u;
    const size_t bin = (size_t)d * nblocks + blockIdx.x;
    unsigned pos = hist[bin] + hblk[bin / kScanBlock] + rank[r];
    for (int q = 0; q < wave; ++q) pos += sub[q][d];
    if (pos >= n) continue;                                    // (a permutation of 0 .. n - 1)
    const unsigned from = idx ? idx[i] : (unsigned)i;
    if (key_out) {
      key_out[pos] = k[r];
      idx_out[pos] = from;
    } else if (from < n) {
      perm[from] = pos;
    }
  }
}

// perm[raster index] = position in label-major order, raster order kept inside a label
int sort_by_label(const unsigned short* key, long long n, int passes, const MeshLabelSortWs& w, unsigned* perm, hipStream_t s) {
  if (n == 0) return 0;
  const unsigned nblocks = (unsigned)((n + kSortBlock - 1) / kSortBlock);
  const long long bins = 256ll * nblocks;
  for (int pass = 0; pass < passes; ++pass) {
    const bool last = pass + 1 == passes;
    const unsigned short* in = pass ? w.key2 : key;
    radix_hist_kernel<<<nblocks, 256, 0, s>>>(in, n, 8 * pass, nblocks, w.hist);
    if (int e = run_scan(w.hist, nullptr, bins, w.hblk, nullptr, w.total, s)) return e;
    radix_scatter_kernel<<<nblocks, 256, 0, s>>>(in, pass ? w.idx2 : nullptr, n, 8 * pass, nblocks, w.hist, w.hblk,
                                                 last ? nullptr : w.key2, last ? nullptr : w.idx2, perm);
  }
  SEUNET_LAUNCH_CHECK();
  return 0;
}

LabelGeom label_geom(int n0, int n1, int n2, int num) {
  LabelGeom g{bit_geom(n0, n1, n2)};
  g.limit = num < 0 ? kMeshLabelMax : num;
  g.cells = n0 >= 2 && n1 >= 2 && n2 >= 2;
  return g;
}

constexpr long long kInt32Max = 0x7fffffffll;

}  // namespace

size_t mesh_label_workspace_bytes(int n0, int n1, int n2) { return measured(mesh_label_ws, n0, n1, n2); }
size_t mesh_label_sort_bytes(long long nverts, long long nfaces) {
  WsCarver c(nullptr);
  mesh_label_sort_ws(c, nverts, nfaces);
  return c.bytes();
}

int launch_mesh_label_count(const int* labels, int n0, int n1, int n2, int num, long long* nverts, long long* nfaces, int* num_used,
                            int* status, long long* vert_ptr_dev, long long* face_ptr_dev, int ptr_capacity, void* workspace,
                            size_t ws_bytes, hipStream_t s) {
  SEUNET_CHECK(labels && nverts && nfaces && num_used && status && vert_ptr_dev && face_ptr_dev && workspace,
               "mesh_label_count: null argument");
  if (int e = volume_check("mesh_label_count", n0, n1, n2, 0)) return e;
  SEUNET_CHECK(num >= -1 && num <= kMeshLabelMax, "mesh_label_count: num %d (-1: the largest label present, at most %d)", num,
               kMeshLabelMax);
  const int need = num < 0 ? kMeshLabelMax + 1 : num + 1;
  SEUNET_CHECK(ptr_capacity >= need, "mesh_label_count: room for %d pointer entries, %d needed", ptr_capacity, need);
  WsCarver carve(workspace);
  const MeshLabelWs w = mesh_label_ws(carve, n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "mesh_label_count: workspace too small (%zu bytes, %zu needed)", ws_bytes, carve.bytes());
  const LabelGeom g = label_geom(n0, n1, n2, num);
  SEUNET_HIP(hipMemsetAsync(w.rec, 0, sizeof(MeshLabelRec), s));
  SEUNET_HIP(hipMemsetAsync(w.vhist, 0, (kMeshLabelMax + 1) * sizeof(unsigned), s));
  SEUNET_HIP(hipMemsetAsync(w.fhist, 0, (kMeshLabelMax + 1) * sizeof(unsigned), s));
  label_count_kernel<<<(unsigned)((g.words + 3) / 4), 256, 0, s>>>(labels, g, w);
  if (int e = run_scan(w.vcnt, w.fcnt, g.words, w.vblk, w.fblk, &w.rec->nverts, s)) return e;
  if (int e = run_scan(w.vhist, w.fhist, kMeshLabelMax + 1, w.hvblk, w.hfblk, w.htotal, s)) return e;
  label_ptr_kernel<<<blocks_256(need), 256, 0, s>>>(w, g.cells, vert_ptr_dev, face_ptr_dev, need);
  SEUNET_LAUNCH_CHECK();
  MeshLabelRec host;                                           // the one synchronisation: sizes, largest label, status
  SEUNET_HIP(hipMemcpyAsync(&host, w.rec, sizeof(MeshLabelRec), hipMemcpyDeviceToHost, s));
  SEUNET_HIP(hipStreamSynchronize(s));
  if (!g.cells) host.nverts = host.nfaces = 0;                 // no cells: empty meshes, vertices included
  *nverts = (long long)host.nverts;
  *nfaces = (long long)host.nfaces;
  *num_used = num < 0 ? host.max_label : num;
  *status = host.status;
  return 0;
}

int launch_mesh_label_emit(const int* labels, int n0, int n1, int n2, int num, double level, long long nverts, long long nfaces,
                           float* verts, int* faces, const void* workspace, size_t ws_bytes, void* sort_workspace, size_t sort_bytes,
                           hipStream_t s) {
  SEUNET_CHECK(labels && workspace, "mesh_label_emit: null argument");
  if (int e = volume_check("mesh_label_emit", n0, n1, n2, 0)) return e;
  SEUNET_CHECK(num >= 0 && num <= kMeshLabelMax, "mesh_label_emit: num %d (0 .. %d, as mesh_label_count returned it)", num, kMeshLabelMax);
  SEUNET_CHECK(level > 0.0 && level < 1.0, "mesh_label_emit: level %g is not strictly between 0 and 1", level);
  SEUNET_CHECK(nverts >= 0 && nfaces >= 0, "mesh_label_emit: negative size");
  SEUNET_CHECK(nverts <= kInt32Max, "mesh_label_emit: %lld vertices exceed the int32 index range", nverts);
  SEUNET_CHECK(3 * nfaces <= kInt32Max, "mesh_label_emit: %lld faces: 3 F exceeds the int32 range", nfaces);
  if (nverts == 0 && nfaces == 0) return 0;
  SEUNET_CHECK(n0 >= 2 && n1 >= 2 && n2 >= 2, "mesh_label_emit: a volume without cells has empty meshes");
  SEUNET_CHECK((nverts == 0 || verts) && (nfaces == 0 || faces) && sort_workspace, "mesh_label_emit: null output or sort workspace");
  WsCarver carve(const_cast<void*>(workspace));
  const MeshLabelWs w = mesh_label_ws(carve, n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "mesh_label_emit: workspace too small (%zu bytes, %zu needed)", ws_bytes, carve.bytes());
  WsCarver carve_sort(sort_workspace);
  const MeshLabelSortWs sw = mesh_label_sort_ws(carve_sort, nverts, nfaces);
  SEUNET_CHECK(sort_bytes >= carve_sort.bytes(), "mesh_label_emit: sort workspace too small (%zu bytes, %zu needed)", sort_bytes,
               carve_sort.bytes());
  const LabelGeom g = label_geom(n0, n1, n2, num);
  const unsigned word_blocks = (unsigned)((g.words + 3) / 4);
  ItemArgs e{};
  e.labels = labels; e.w = w; e.nverts = nverts; e.nfaces = nfaces;
  e.vkey = sw.vkey; e.fkey = sw.fkey;
  label_items_kernel<true><<<word_blocks, 256, 0, s>>>(e, g);
  const int passes = num < 256 ? 1 : 2;
  if (int err = sort_by_label(sw.vkey, nverts, passes, sw, sw.vperm, s)) return err;
  if (int err = sort_by_label(sw.fkey, nfaces, passes, sw, sw.fperm, s)) return err;
  e.vperm = sw.vperm; e.fperm = sw.fperm;
  e.t_lo0 = (float)level;                                      // formed in float64, rounded once
  e.t_lo1 = (float)(1.0 - level);
  e.verts = verts; e.faces = faces;
  label_items_kernel<false><<<word_blocks, 256, 0, s>>>(e, g);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
