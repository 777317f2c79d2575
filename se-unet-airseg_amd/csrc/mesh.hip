// Surface meshing on the device: a 0/1 volume to an indexed triangle mesh, its vertex adjacency, Jacobi
// smoothing, the affine step and binary-STL records.
//
// Reference (CPU): prediction.py:121-149 -- marching_cubes_lewiner(result, 0.95), centring on the skeleton's mean, scaling by
// spacing / 10, a Python loop over the faces into an STL and pyvista's smooth(relaxation_factor=0.2).  Equality with Lewiner's
// triangulation or with VTK's smoothing is not claimed; the definition implemented here is written out in DESIGN.md 3h and,
// executably, in tests/mesh_oracle.py, and every result below equals that oracle bit for bit.
//
// Extraction.  The volume is bit-packed along the last axis (bitvol.h; pack_bits and run_scan are that
// layer's).  One wavefront works on one word, one lane per voxel / cell:
//   count  the three masks of owned vertices of the word (voxel differs from its +1 neighbour along axis 0 / 1 / 2) are word
//          operations, their popcounts the word's vertex count; a lane's cell configuration comes from the words of the 2 x 2
//          neighbouring rows, its triangle count from the table, the word's total from ballots of the count's three bits.  A word
//          whose 2 x 2 rows are all 0 or all 1 is left after the loads.
//   scan   block-wise exclusive scan of the per-word counts in place, then one workgroup over the block totals: no atomics, the
//          numbering cannot depend on scheduling.  The two totals go to a record the host reads once (the one synchronisation).
//   emit   vertex index = word base + popcount of the owned masks below the lane (+ the lane's earlier axes); face index = word
//          base + ballot rank; a triangle corner on cube edge e looks up the word that owns that grid edge.
// Adjacency.  Every face corner adds its two neighbours, tagged outgoing / incoming, to the corner's list (integer atomics pick
// the slot); each list is then sorted and stripped of repeats, so the result is independent of the slot order.  A neighbour that
// appears with one tag only is a directed edge without its reverse: both ends are boundary vertices.
// Arithmetic.  Every float32 operation of the smoothing, the affine step and the normals is a single correctly rounded operation
// in a fixed order (this file is compiled with -ffp-contract=off; division and square root are the correctly rounded ones).
#include "volume.h"
#include "mesh_table.h"
#include <math.h>

namespace seunet {

namespace {

__constant__ MeshTable kTable = make_mesh_table();

// ---- extraction ----------------------------------------------------------------------------------------------------------------
// What a wavefront needs of the 2 x 2 rows around its word: the four words, each shifted down by one voxel (bit b = voxel b + 1,
// bit 63 from the next word), and the lanes whose voxel has a +1 neighbour along axis 2.
struct CellWords {
  u64 m00, m01, m10, m11;     // rows (i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1); 0 where the row does not exist
  u64 s00, s01, s10, s11;
  u64 valid2;
  bool has0, has1;
  bool flat;                  // all eight are all-0 or all-1: no vertex, no triangle
};

__device__ __forceinline__ CellWords load_cell_words(const u64* __restrict__ bits, const BitGeom& g, long long t) {
  CellWords c;
  const int w = (int)(t % g.W);
  const long long row = t / g.W;
  const int j = (int)(row % g.n1), i = (int)(row / g.n1);
  c.has0 = i + 1 < g.n0;
  c.has1 = j + 1 < g.n1;
  const bool more = w + 1 < g.W;
  const long long d0 = (long long)g.n1 * g.W, d1 = g.W;
  c.m00 = bits[t];
  c.m01 = c.has1 ? bits[t + d1] : 0ull;
  c.m10 = c.has0 ? bits[t + d0] : 0ull;
  c.m11 = c.has0 && c.has1 ? bits[t + d0 + d1] : 0ull;
  const u64 x00 = more ? bits[t + 1] : 0ull;
  const u64 x01 = more && c.has1 ? bits[t + d1 + 1] : 0ull;
  const u64 x10 = more && c.has0 ? bits[t + d0 + 1] : 0ull;
  const u64 x11 = more && c.has0 && c.has1 ? bits[t + d0 + d1 + 1] : 0ull;
  c.s00 = shift_up(c.m00, x00);
  c.s01 = shift_up(c.m01, x01);
  c.s10 = shift_up(c.m10, x10);
  c.s11 = shift_up(c.m11, x11);
  c.valid2 = shift_up(tail_mask(g, w), more ? 1ull : 0ull);  // the voxels whose successor is a voxel of the row
  const u64 any = c.m00 | c.m01 | c.m10 | c.m11 | ((x00 | x01 | x10 | x11) & 1ull);
  const u64 all = c.m00 & c.m01 & c.m10 & c.m11;
  c.flat = any == 0ull || (all == ~0ull && (x00 & x01 & x10 & x11 & 1ull) != 0ull);
  return c;
}

// masks of the vertices the word's voxels own along axis 0, 1, 2
__device__ __forceinline__ void owned_masks(const CellWords& c, u64& a0, u64& a1, u64& a2) {
  a0 = c.has0 ? c.m00 ^ c.m10 : 0ull;
  a1 = c.has1 ? c.m00 ^ c.m01 : 0ull;
  a2 = (c.m00 ^ c.s00) & c.valid2;
}

// triangles of this lane's cell (0 where the lane has no cell); cfg receives the configuration
__device__ __forceinline__ int cell_triangles(const CellWords& c, int lane, int& cfg) {
  cfg = 0;
  if (!(c.has0 && c.has1 && ((c.valid2 >> lane) & 1ull))) return 0;
  cfg = (int)(((c.m00 >> lane) & 1ull) | (((c.s00 >> lane) & 1ull) << 1) | (((c.m01 >> lane) & 1ull) << 2) |
              (((c.s01 >> lane) & 1ull) << 3) | (((c.m10 >> lane) & 1ull) << 4) | (((c.s10 >> lane) & 1ull) << 5) |
              (((c.m11 >> lane) & 1ull) << 6) | (((c.s11 >> lane) & 1ull) << 7));
  return kTable.count[cfg];
}

__global__ void __launch_bounds__(256)
mesh_count_kernel(const u64* __restrict__ bits, BitGeom g, u64* __restrict__ a0s, u64* __restrict__ a1s, u64* __restrict__ a2s,
                  unsigned* __restrict__ vcnt, unsigned* __restrict__ fcnt) {
  const long long t = (blockIdx.x * 256ll + threadIdx.x) >> 6;
  if (t >= g.words) return;
  const int lane = threadIdx.x & 63;
  const CellWords c = load_cell_words(bits, g, t);
  u64 a0 = 0ull, a1 = 0ull, a2 = 0ull;
  unsigned nf = 0u;
  if (!c.flat) {                                             // uniform; most words of a CT are empty
    owned_masks(c, a0, a1, a2);
    int cfg;
    const int n = cell_triangles(c, lane, cfg);
    nf = (unsigned)ballot_sum<3>(n);
  }
  if (lane == 0) {
    a0s[t] = a0;
    a1s[t] = a1;
    a2s[t] = a2;
    vcnt[t] = (unsigned)(__popcll(a0) + __popcll(a1) + __popcll(a2));
    fcnt[t] = nf;
  }
}

struct EmitArgs {
  const u64 *bits, *a0s, *a1s, *a2s;
  const unsigned *vcnt, *fcnt, *vblk, *fblk;                 // after the scan: exclusive within a block, exclusive block bases
  float t_lo0, t_lo1;                                        // offset of a vertex whose low end is 0 / 1
  long long nverts, nfaces;
  float* verts;
  int* faces;
};

__device__ __forceinline__ void put_vertex(const EmitArgs& e, long long idx, float x0, float x1, float x2) {
  if (idx >= e.nverts) return;                               // (cannot happen with the totals of the count pass)
  float* p = e.verts + idx * 3;
  p[0] = x0; p[1] = x1; p[2] = x2;
}

// index of the vertex on cube edge `edge` of the cell at (i, j, k)
__device__ __forceinline__ int edge_vertex(const EmitArgs& e, const BitGeom& g, int i, int j, int k, int edge) {
  const int axis = edge >> 2, du = (edge >> 1) & 1, dv = edge & 1;
  const int d0 = axis == 0 ? 0 : du, d1 = axis == 0 ? du : (axis == 1 ? 0 : dv), d2 = axis == 2 ? 0 : dv;
  const int kk = k + d2;
  const long long tw = ((long long)(i + d0) * g.n1 + (j + d1)) * g.W + (kk >> 6);
  const int bit = kk & 63;
  const u64 below = (1ull << bit) - 1ull;
  const u64 a0 = e.a0s[tw], a1 = e.a1s[tw], a2 = e.a2s[tw];
  unsigned id = e.vblk[tw / kScanBlock] + e.vcnt[tw] + (unsigned)(__popcll(a0 & below) + __popcll(a1 & below) + __popcll(a2 & below));
  if (axis > 0) id += (unsigned)((a0 >> bit) & 1ull);
  if (axis > 1) id += (unsigned)((a1 >> bit) & 1ull);
  return (int)id;
}

__global__ void __launch_bounds__(256) mesh_emit_kernel(EmitArgs e, BitGeom g) {
  const long long t = (blockIdx.x * 256ll + threadIdx.x) >> 6;
  if (t >= g.words) return;
  const int lane = threadIdx.x & 63;
  const CellWords c = load_cell_words(e.bits, g, t);
  if (c.flat) return;                                        // uniform
  const int w = (int)(t % g.W);
  const long long row = t / g.W;
  const int j = (int)(row % g.n1), i = (int)(row / g.n1), k = 64 * w + lane;
  const u64 below = (1ull << lane) - 1ull;

  u64 a0, a1, a2;
  owned_masks(c, a0, a1, a2);
  if ((a0 | a1 | a2) != 0ull) {
    long long idx = (long long)(e.vblk[t / kScanBlock] + e.vcnt[t]) + __popcll(a0 & below) + __popcll(a1 & below) + __popcll(a2 & below);
    const float tt = ((c.m00 >> lane) & 1ull) ? e.t_lo1 : e.t_lo0;
    const float f0 = (float)i, f1 = (float)j, f2 = (float)k;
    if ((a0 >> lane) & 1ull) put_vertex(e, idx++, __fadd_rn(f0, tt), f1, f2);
    if ((a1 >> lane) & 1ull) put_vertex(e, idx++, f0, __fadd_rn(f1, tt), f2);
    if ((a2 >> lane) & 1ull) put_vertex(e, idx++, f0, f1, __fadd_rn(f2, tt));
  }

  int cfg;
  const int n = cell_triangles(c, lane, cfg);
  const BitPlanes<3> nb = ballot_planes<3>(n);
  if ((nb.b[0] | nb.b[1] | nb.b[2]) == 0ull) return;
  const long long first = (long long)(e.fblk[t / kScanBlock] + e.fcnt[t]) + plane_sum(nb, below);
  for (int q = 0; q < n; ++q) {
    const long long f = first + q;
    if (f >= e.nfaces) break;                                // (cannot happen with the totals of the count pass)
#pragma unroll
    for (int corner = 0; corner < 3; ++corner) e.faces[f * 3 + corner] = edge_vertex(e, g, i, j, k, kTable.edges[cfg][3 * q + corner]);
  }
}

// ---- skeleton centre: exact integer sums ----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) mesh_coord_sums_kernel(const unsigned char* __restrict__ mask, long long n, int n1, int n2, u64* out) {
  u64 cnt = 0ull, s0 = 0ull, s1 = 0ull, s2 = 0ull;
  for (long long v = blockIdx.x * 256ll + threadIdx.x; v < n; v += gridDim.x * 256ll)
    if (mask[v] != 0) {
      const Vox3 p = vox3(v, n1, n2);
      ++cnt;
      s0 += (u64)p.i0; s1 += (u64)p.i1; s2 += (u64)p.i2;
    }
  cnt = wave_sum(cnt); s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
  if ((threadIdx.x & 63) == 0 && cnt != 0ull) {              // integer additions: the order of the atomics cannot matter
    atomicAdd(&out[0], cnt); atomicAdd(&out[1], s0); atomicAdd(&out[2], s1); atomicAdd(&out[3], s2);
  }
}

// ---- adjacency ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool load_face(const int* __restrict__ faces, long long f, unsigned V, int (&v)[3]) {
  v[0] = faces[f * 3]; v[1] = faces[f * 3 + 1]; v[2] = faces[f * 3 + 2];
  return (unsigned)v[0] < V && (unsigned)v[1] < V && (unsigned)v[2] < V;
}

__global__ void __launch_bounds__(256)
adj_degree_kernel(const int* __restrict__ faces, long long F, unsigned V, unsigned* deg, int* status) {
  const long long f = blockIdx.x * 256ll + threadIdx.x;
  if (f >= F) return;
  int v[3];
  if (!load_face(faces, f, V, v)) { *status = 1; return; }    // an index outside [0, V): reported, the face is left out
#pragma unroll
  for (int q = 0; q < 3; ++q) atomicAdd(&deg[v[q]], 2u);
}

__global__ void __launch_bounds__(256)
adj_fill_kernel(const int* __restrict__ faces, long long F, unsigned V, const unsigned* __restrict__ rawptr, unsigned* cursor,
                unsigned* __restrict__ raw) {
  const long long f = blockIdx.x * 256ll + threadIdx.x;
  if (f >= F) return;
  int v[3];
  if (!load_face(faces, f, V, v)) return;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const unsigned at = rawptr[v[q]] + atomicAdd(&cursor[v[q]], 2u);
    raw[at] = (unsigned)v[(q + 1) % 3] << 1;                   // the edge that leaves this corner
    raw[at + 1] = ((unsigned)v[(q + 2) % 3] << 1) | 1u;        // the edge that arrives
  }
}

// one thread per vertex: sort its short list, keep each neighbour once at the front of the list, count, flag
__global__ void __launch_bounds__(256)
adj_sort_kernel(unsigned V, const unsigned* __restrict__ rawptr, unsigned* __restrict__ raw, unsigned* __restrict__ deg,
                unsigned char* __restrict__ boundary) {
  const long long v = blockIdx.x * 256ll + threadIdx.x;
  if (v >= V) return;
  const unsigned lo = rawptr[v], hi = rawptr[v + 1];
  for (unsigned a = lo + 1; a < hi; ++a) {                    // insertion sort
    const unsigned key = raw[a];
    unsigned b = a;
    while (b > lo && raw[b - 1] > key) { raw[b] = raw[b - 1]; --b; }
    raw[b] = key;
  }
  unsigned out = lo, at = lo;
  bool open = false;
  while (at < hi) {
    const unsigned nb = raw[at] >> 1;
    bool leaves = false, arrives = false;
    while (at < hi && (raw[at] >> 1) == nb) {
      if (raw[at] & 1u) arrives = true; else leaves = true;
      ++at;
    }
    raw[out++] = nb;                                          // out <= the entries already read
    open = open || leaves != arrives;
  }
  deg[v] = out - lo;
  boundary[v] = open ? 1 : 0;
}

__global__ void __launch_bounds__(256)
adj_compact_kernel(unsigned V, const unsigned* __restrict__ rawptr, const unsigned* __restrict__ raw, const int* __restrict__ indptr,
                   int* __restrict__ indices, long long capacity) {
  const long long v = blockIdx.x * 256ll + threadIdx.x;
  if (v >= V) return;
  const long long first = indptr[v], n = indptr[v + 1] - first;
  const unsigned lo = rawptr[v];
  for (long long q = 0; q < n && first + q < capacity; ++q) indices[first + q] = (int)raw[lo + q];
}

// ---- smoothing, affine step, STL records -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
mesh_smooth_kernel(const float* __restrict__ x, long long V, const int* __restrict__ indptr, const int* __restrict__ indices,
                   const unsigned char* __restrict__ boundary, float lambda, float* __restrict__ out) {
  const long long v = blockIdx.x * 256ll + threadIdx.x;
  if (v >= V) return;
  const float p0 = x[v * 3], p1 = x[v * 3 + 1], p2 = x[v * 3 + 2];
  const int lo = indptr[v], hi = indptr[v + 1];
  float r0 = p0, r1 = p1, r2 = p2;
  if (hi > lo && boundary[v] == 0) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int q = lo; q < hi; ++q) {                           // ascending neighbour index
      const float* n = x + (long long)indices[q] * 3;
      s0 = __fadd_rn(s0, n[0]); s1 = __fadd_rn(s1, n[1]); s2 = __fadd_rn(s2, n[2]);
    }
    const float d = (float)(hi - lo);
    r0 = __fadd_rn(p0, __fmul_rn(lambda, __fsub_rn(__fdiv_rn(s0, d), p0)));
    r1 = __fadd_rn(p1, __fmul_rn(lambda, __fsub_rn(__fdiv_rn(s1, d), p1)));
    r2 = __fadd_rn(p2, __fmul_rn(lambda, __fsub_rn(__fdiv_rn(s2, d), p2)));
  }
  out[v * 3] = r0; out[v * 3 + 1] = r1; out[v * 3 + 2] = r2;
}

struct Affine { float c[3], s[3]; };
__device__ __forceinline__ float affine1(const Affine& a, int axis, float v) { return __fmul_rn(__fsub_rn(v, a.c[axis]), a.s[axis]); }

__global__ void __launch_bounds__(256) mesh_affine_kernel(const float* __restrict__ x, long long n3, Affine a, float* __restrict__ out) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i < n3) out[i] = affine1(a, (int)(i % 3), x[i]);
}

__global__ void __launch_bounds__(256)
mesh_stl_kernel(const float* __restrict__ x, unsigned V, const int* __restrict__ faces, long long F, Affine a,
                unsigned short* __restrict__ rec, int* status) {
  const long long f = blockIdx.x * 256ll + threadIdx.x;
  if (f >= F) return;
  float r[12];
  int v[3];
  if (load_face(faces, f, V, v)) {
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) r[3 + 3 * q + ax] = affine1(a, ax, x[(long long)v[q] * 3 + ax]);
    const float u0 = __fsub_rn(r[6], r[3]), u1 = __fsub_rn(r[7], r[4]), u2 = __fsub_rn(r[8], r[5]);
    const float w0 = __fsub_rn(r[9], r[3]), w1 = __fsub_rn(r[10], r[4]), w2 = __fsub_rn(r[11], r[5]);
    const float n0 = __fsub_rn(__fmul_rn(u1, w2), __fmul_rn(u2, w1));
    const float n1 = __fsub_rn(__fmul_rn(u2, w0), __fmul_rn(u0, w2));
    const float n2 = __fsub_rn(__fmul_rn(u0, w1), __fmul_rn(u1, w0));
    const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(n0, n0), __fmul_rn(n1, n1)), __fmul_rn(n2, n2)));
    const bool area = len > 0.f;
    r[0] = area ? __fdiv_rn(n0, len) : 0.f;
    r[1] = area ? __fdiv_rn(n1, len) : 0.f;
    r[2] = area ? __fdiv_rn(n2, len) : 0.f;
  } else {
    *status = 1;                                              // an index outside [0, V): reported, a zero record
#pragma unroll
    for (int q = 0; q < 12; ++q) r[q] = 0.f;
  }
  unsigned short* p = rec + f * 25;                           // 50-byte records: 2-byte alignment only
#pragma unroll
  for (int q = 0; q < 12; ++q) {
    const unsigned bitsq = __float_as_uint(r[q]);
    p[2 * q] = (unsigned short)(bitsq & 0xffffu);
    p[2 * q + 1] = (unsigned short)(bitsq >> 16);
  }
  p[24] = 0;
}

int make_affine(const float* centre, const float* scale, Affine* a) {
  for (int q = 0; q < 3; ++q) {
    a->c[q] = centre ? centre[q] : 0.f;
    a->s[q] = scale ? scale[q] : 1.f;
  }
  return 0;
}

constexpr long long kInt32Max = 0x7fffffffll;

}  // namespace

size_t mesh_workspace_bytes(int n0, int n1, int n2) { return measured(mesh_ws, n0, n1, n2); }
size_t mesh_adjacency_workspace_bytes(long long nverts, long long nfaces) {
  WsCarver c(nullptr);
  mesh_adj_ws(c, nverts, nfaces);
  return c.bytes();
}

int launch_mesh_count(const unsigned char* vol, int n0, int n1, int n2, long long* nverts, long long* nfaces, void* workspace,
                      size_t ws_bytes, hipStream_t s) {
  SEUNET_CHECK(vol && nverts && nfaces && workspace, "mesh_count: null argument");
  if (int e = volume_check("mesh_count", n0, n1, n2, 0)) return e;
  WsCarver carve(workspace);
  const MeshWs w = mesh_ws(carve, n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "mesh_count: workspace too small (%zu bytes, %zu needed)", ws_bytes, carve.bytes());
  const BitGeom g = bit_geom(n0, n1, n2);
  const unsigned word_blocks = (unsigned)((g.words + 3) / 4);
  pack_bits(vol, nullptr, g, w.bits, nullptr, s);
  mesh_count_kernel<<<word_blocks, 256, 0, s>>>(w.bits, g, w.a0, w.a1, w.a2, w.vcnt, w.fcnt);
  if (int e = run_scan(w.vcnt, w.fcnt, g.words, w.vblk, w.fblk, &w.rec->nverts, s)) return e;
  MeshRec host;                                                // the one synchronisation of the extraction: the output sizes
  SEUNET_HIP(hipMemcpyAsync(&host, w.rec, sizeof(MeshRec), hipMemcpyDeviceToHost, s));
  SEUNET_HIP(hipStreamSynchronize(s));
  if (n0 < 2 || n1 < 2 || n2 < 2) host.nverts = host.nfaces = 0;   // no cells: an empty mesh, vertices included
  *nverts = (long long)host.nverts;
  *nfaces = (long long)host.nfaces;
  return 0;
}

int launch_mesh_emit(int n0, int n1, int n2, double level, long long nverts, long long nfaces, float* verts, int* faces,
                     const void* workspace, size_t ws_bytes, hipStream_t s) {
  SEUNET_CHECK(workspace, "mesh_emit: null workspace");
  if (int e = volume_check("mesh_emit", n0, n1, n2, 0)) return e;
  SEUNET_CHECK(level > 0.0 && level < 1.0, "mesh_emit: level %g is not strictly between 0 and 1", level);
  SEUNET_CHECK(nverts >= 0 && nfaces >= 0, "mesh_emit: negative size");
  SEUNET_CHECK(nverts <= kInt32Max, "mesh_emit: %lld vertices exceed the int32 index range", nverts);
  SEUNET_CHECK(3 * nfaces <= kInt32Max, "mesh_emit: %lld faces: 3 F exceeds the int32 range", nfaces);
  if (nverts == 0 && nfaces == 0) return 0;
  SEUNET_CHECK(n0 >= 2 && n1 >= 2 && n2 >= 2, "mesh_emit: a volume without cells has an empty mesh");
  SEUNET_CHECK((nverts == 0 || verts) && (nfaces == 0 || faces), "mesh_emit: null output");
  WsCarver carve(const_cast<void*>(workspace));
  const MeshWs w = mesh_ws(carve, n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "mesh_emit: workspace too small (%zu bytes, %zu needed)", ws_bytes, carve.bytes());
  const BitGeom g = bit_geom(n0, n1, n2);
  EmitArgs e;
  e.bits = w.bits; e.a0s = w.a0; e.a1s = w.a1; e.a2s = w.a2;
  e.vcnt = w.vcnt; e.fcnt = w.fcnt; e.vblk = w.vblk; e.fblk = w.fblk;
  e.t_lo0 = (float)level;                                      // formed in float64, rounded once
  e.t_lo1 = (float)(1.0 - level);
  e.nverts = nverts; e.nfaces = nfaces; e.verts = verts; e.faces = faces;
  mesh_emit_kernel<<<(unsigned)((g.words + 3) / 4), 256, 0, s>>>(e, g);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_mesh_coord_sums(const unsigned char* mask, int n0, int n1, int n2, long long* sums_dev, hipStream_t s) {
  SEUNET_CHECK(mask && sums_dev, "mesh_coord_sums: null argument");
  if (int e = volume_check("mesh_coord_sums", n0, n1, n2, 0)) return e;
  const long long n = (long long)n0 * n1 * n2;
  SEUNET_HIP(hipMemsetAsync(sums_dev, 0, 4 * sizeof(long long), s));
  mesh_coord_sums_kernel<<<grid_for(n), 256, 0, s>>>(mask, n, n1, n2, reinterpret_cast<u64*>(sums_dev));
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_mesh_adjacency(const int* faces, long long nfaces, long long nverts, int* indptr, int* indices, long long capacity,
                          unsigned char* boundary, int* status_dev, void* workspace, size_t ws_bytes, hipStream_t s) {
  SEUNET_CHECK(indptr && status_dev && workspace, "mesh_adjacency: null argument");
  SEUNET_CHECK(nverts >= 0 && nfaces >= 0 && nverts <= kInt32Max - 1, "mesh_adjacency: %lld vertices (0 .. 2^31-2)", nverts);
  SEUNET_CHECK(6 * nfaces <= kInt32Max, "mesh_adjacency: %lld faces: 6 F exceeds the int32 range", nfaces);
  SEUNET_CHECK(capacity >= 6 * nfaces, "mesh_adjacency: room for %lld neighbour indices, 6 F = %lld needed", capacity, 6 * nfaces);
  SEUNET_CHECK((nfaces == 0 || (faces && indices)) && (nverts == 0 || boundary), "mesh_adjacency: null argument");
  WsCarver carve(workspace);
  const MeshAdjWs w = mesh_adj_ws(carve, nverts, nfaces);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "mesh_adjacency: workspace too small (%zu bytes, %zu needed)", ws_bytes, carve.bytes());
  const unsigned V = (unsigned)nverts;
  SEUNET_HIP(hipMemsetAsync(status_dev, 0, sizeof(int), s));
  SEUNET_HIP(hipMemsetAsync(w.deg, 0, (size_t)(nverts + 1) * sizeof(unsigned), s));
  if (nfaces > 0) adj_degree_kernel<<<blocks_256(nfaces), 256, 0, s>>>(faces, nfaces, V, w.deg, status_dev);
  if (int e = run_scan(w.deg, nullptr, nverts, w.blk, nullptr, w.total, s)) return e;
  scan_add(w.deg, w.blk, nverts, w.total, w.rawptr, s);
  SEUNET_HIP(hipMemsetAsync(w.deg, 0, (size_t)(nverts + 1) * sizeof(unsigned), s));     // now the fill cursors
  if (nfaces > 0) adj_fill_kernel<<<blocks_256(nfaces), 256, 0, s>>>(faces, nfaces, V, w.rawptr, w.deg, w.raw);
  if (nverts > 0) adj_sort_kernel<<<blocks_256(nverts), 256, 0, s>>>(V, w.rawptr, w.raw, w.deg, boundary);   // deg: the final degrees
  if (int e = run_scan(w.deg, nullptr, nverts, w.blk, nullptr, w.total, s)) return e;
  scan_add(w.deg, w.blk, nverts, w.total, reinterpret_cast<unsigned*>(indptr), s);
  if (nverts > 0 && nfaces > 0) adj_compact_kernel<<<blocks_256(nverts), 256, 0, s>>>(V, w.rawptr, w.raw, indptr, indices, capacity);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_mesh_smooth(const float* verts, long long nverts, const int* indptr, const int* indices, const unsigned char* boundary,
                       int n_iter, float relaxation, float* out, float* tmp, hipStream_t s) {
  SEUNET_CHECK(nverts >= 0 && nverts <= kInt32Max && n_iter >= 0, "mesh_smooth: bad argument");
  if (nverts == 0) return 0;
  SEUNET_CHECK(verts && indptr && boundary && out && out != verts, "mesh_smooth: null argument, or out aliases verts");
  SEUNET_CHECK(n_iter < 2 || (tmp && tmp != verts && tmp != out), "mesh_smooth: more than one sweep needs a second buffer");
  if (n_iter == 0) {
    SEUNET_HIP(hipMemcpyAsync(out, verts, (size_t)nverts * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
  }
  const float* src = verts;
  for (int sweep = 1; sweep <= n_iter; ++sweep) {              // double-buffered; the last sweep writes `out`
    float* dst = (n_iter - sweep) % 2 == 0 ? out : tmp;
    mesh_smooth_kernel<<<blocks_256(nverts), 256, 0, s>>>(src, nverts, indptr, indices, boundary, relaxation, dst);
    src = dst;
  }
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_mesh_affine(const float* verts, long long nverts, const float* centre, const float* scale, float* out, hipStream_t s) {
  SEUNET_CHECK(nverts >= 0 && nverts <= kInt32Max, "mesh_affine: bad vertex count %lld", nverts);
  if (nverts == 0) return 0;
  SEUNET_CHECK(verts && out, "mesh_affine: null argument");
  Affine a;
  make_affine(centre, scale, &a);
  mesh_affine_kernel<<<blocks_256(nverts * 3), 256, 0, s>>>(verts, nverts * 3, a, out);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_mesh_stl_records(const float* verts, long long nverts, const int* faces, long long nfaces, const float* centre,
                            const float* scale, unsigned char* records, int* status_dev, hipStream_t s) {
  SEUNET_CHECK(status_dev, "mesh_stl_records: null status");
  SEUNET_CHECK(nverts >= 0 && nverts <= kInt32Max && nfaces >= 0 && 3 * nfaces <= kInt32Max, "mesh_stl_records: bad sizes (%lld, %lld)",
               nverts, nfaces);
  SEUNET_HIP(hipMemsetAsync(status_dev, 0, sizeof(int), s));
  if (nfaces == 0) return 0;
  SEUNET_CHECK(faces && records && (nverts == 0 || verts), "mesh_stl_records: null argument");
  SEUNET_CHECK((reinterpret_cast<uintptr_t>(records) & 1u) == 0, "mesh_stl_records: the record buffer must be 2-byte aligned");
  Affine a;
  make_affine(centre, scale, &a);
  mesh_stl_kernel<<<blocks_256(nfaces), 256, 0, s>>>(verts, (unsigned)nverts, faces, nfaces, a, reinterpret_cast<unsigned short*>(records),
                                                     status_dev);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
