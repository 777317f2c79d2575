// The bit-packed volume layer that morph.hip, dti.hip, skeleton.hip, mesh.hip, mesh_label.hip,
// surface.hip and betti.hip share: geometry, byte <-> bit packing, neighbour words, the exclusive scan and the wave counts by bit planes.
//
// Representation: 64 voxels of a row (axis 2) per u64, bit b of word w of a row = voxel 64 w + b.  Zero-tail rule: the bits of a
// row's last word past the row's end are 0 in every packed volume, and every kernel that writes one keeps them 0.  The padded form
// (skeleton.hip) adds one zero word on either side of a row, one zero row on either side of axis 1 and one zero plane on either
// side of axis 0, so that a neighbour access needs no bounds test.
#pragma once
#include "seunet_common.h"

namespace seunet {

typedef unsigned long long u64;

// ---- geometry ---------------------------------------------------------------------------------------------------------------
struct BitGeom {
  int n0, n1, n2, W;          // W = words per row
  long long words;            // n0 * n1 * W words that hold voxels
  long long row_stride;       // words from a row to the next: W, padded W + 2
  long long plane_stride;     // rows from a plane to the next: n1, padded n1 + 2
  int pad;                    // 1: the padded form
};

static inline int words_per_row(int n2) { return (n2 + 63) / 64; }
// words of a packed (n0, n1, n2) volume, unpadded
static inline size_t words(int n0, int n1, int n2) { return (size_t)n0 * n1 * words_per_row(n2); }

static inline BitGeom bit_geom(int n0, int n1, int n2, int pad = 0) {
  BitGeom g;
  g.n0 = n0; g.n1 = n1; g.n2 = n2; g.W = words_per_row(n2);
  g.words = (long long)n0 * n1 * g.W;
  g.row_stride = g.W + (pad ? 2 : 0);
  g.plane_stride = (long long)n1 + (pad ? 2 : 0);
  g.pad = pad ? 1 : 0;
  return g;
}
// words of the padded array (padded form only)
static inline unsigned long long padded_words(const BitGeom& g) {
  return (unsigned long long)(g.n0 + 2ll) * g.plane_stride * g.row_stride;
}

// Exclusive scan of a (and b, null: none) over n elements: in place inside blocks of kScanBlock elements, the blocks' totals to
// blk_a / blk_b and scanned there, the grand totals in 64 bits to total[0] / total[1].  Element i's scan value is
// a[i] + blk_a[i / kScanBlock].  No atomics: the numbering cannot depend on scheduling.
constexpr int kScanBlock = 1024;          // elements per workgroup of the block scan: 256 threads x 4
int run_scan(unsigned* a, unsigned* b, long long n, unsigned* blk_a, unsigned* blk_b, u64* total, hipStream_t s);
// out[i] = a[i] + blk[i / kScanBlock] for i < n, out[n] = total[0]: the plain exclusive-scan array (CSR pointers) after run_scan
void scan_add(const unsigned* a, const unsigned* blk, long long n, const u64* total, unsigned* out, hipStream_t s);

// bytes (non-zero = 1) -> bits of a, and of b (null: none) in the same launch; writes the g.words voxel words through word_index
void pack_bits(const unsigned char* a, const unsigned char* b, const BitGeom& g, u64* out_a, u64* out_b, hipStream_t s);
// bits -> bytes 0 / 1, one thread per voxel in both forms (for the thinning a change from one wave per word: DESIGN.md 3n)
void unpack_bits(const u64* bits, const BitGeom& g, unsigned char* out, hipStream_t s);

// word w of row `row` (= i0 * n1 + i1) -> its index in the padded array
__device__ __forceinline__ long long padded_index(const BitGeom& g, long long row, int w) {
  const long long j = row % g.n1, i = row / g.n1;
  return ((i + 1) * g.plane_stride + (j + 1)) * g.row_stride + (w + 1);
}
// t-th voxel word (raster order) -> its index in the array
__device__ __forceinline__ long long word_index(const BitGeom& g, long long t) {
  return g.pad ? padded_index(g, t / g.W, (int)(t % g.W)) : t;
}

// the valid bits of word w of a row: all but the tail of the last word
__device__ __forceinline__ u64 tail_mask(const BitGeom& g, int w) {
  return (w + 1 < g.W || (g.n2 & 63) == 0) ? ~0ull : ((1ull << (g.n2 & 63)) - 1ull);
}

// ---- neighbour words ----------------------------------------------------------------------------------------------------------
// bit b = voxel b + 1 of cur (bit 63 from the next word) / voxel b - 1 (bit 0 from the previous word)
__device__ __forceinline__ u64 shift_up(u64 cur, u64 next) { return (cur >> 1) | (next << 63); }
__device__ __forceinline__ u64 shift_down(u64 cur, u64 prev) { return (cur << 1) | (prev >> 63); }

// A word and the words of its voxels' six face neighbours: bit b of `down` / `up` = voxel b - 1 / b + 1 of the row, r0 / r1 the
// same word of rows i1 - 1 / i1 + 1, p0 / p1 of planes i0 - 1 / i0 + 1.  A neighbour outside the volume reads as `outside` (0 or
// ~0), and so does the tail of a row's last word in x, down and up; r0 .. p1 are the stored words (zero tails).  `valid` =
// tail_mask: a result is masked with it before it is stored.
struct Cross6 { u64 x, down, up, r0, r1, p0, p1, valid; };
__device__ __forceinline__ u64 and6(const Cross6& c) { return c.x & c.down & c.up & c.r0 & c.r1 & c.p0 & c.p1; }
__device__ __forceinline__ u64 or6(const Cross6& c) { return c.x | c.down | c.up | c.r0 | c.r1 | c.p0 | c.p1; }

__device__ __forceinline__ Cross6 load_cross6(const u64* __restrict__ in, const BitGeom& g, long long idx, u64 outside) {
  Cross6 c;
  const long long row = idx / g.W;
  const int m = (int)(idx % g.W);
  const int i1 = (int)(row % g.n1), i0 = (int)(row / g.n1);
  const long long p = word_index(g, idx), plane = g.plane_stride * g.row_stride;
  c.valid = tail_mask(g, m);
  c.x = in[p] | (outside & ~c.valid);                                   // the tail reads as the outside value
  c.down = shift_down(c.x, m > 0 ? in[p - 1] : outside);                // voxel 64 m - 1
  c.up = shift_up(c.x, m + 1 < g.W ? in[p + 1] : outside);              // voxel 64 m + 64 (bit 0 of the next word is always valid)
  c.r0 = i1 > 0 ? in[p - g.row_stride] : outside;
  c.r1 = i1 + 1 < g.n1 ? in[p + g.row_stride] : outside;
  c.p0 = i0 > 0 ? in[p - plane] : outside;
  c.p1 = i0 + 1 < g.n0 ? in[p + plane] : outside;
  return c;
}

// ---- wave counts by bit planes ----------------------------------------------------------------------------------------------------
// Bit plane p of a per-lane count n < 2^PLANES: bit l of b[p] = bit p of lane l's n.  All 64 lanes call.
template <int PLANES> struct BitPlanes { u64 b[PLANES]; };
template <int PLANES> __device__ __forceinline__ BitPlanes<PLANES> ballot_planes(int n) {
  BitPlanes<PLANES> v;
#pragma unroll
  for (int p = 0; p < PLANES; ++p) v.b[p] = __ballot(n & (1 << p));
  return v;
}
// sum of the counts of the lanes in `lanes`
template <int PLANES> __device__ __forceinline__ int plane_sum(const BitPlanes<PLANES>& v, u64 lanes = ~0ull) {
  int s = 0;
#pragma unroll
  for (int p = 0; p < PLANES; ++p) s += __popcll(v.b[p] & lanes) << p;
  return s;
}
__device__ __forceinline__ u64 lanes_below(int lane) { return (1ull << lane) - 1ull; }
// sum of n over the wave.  The ranked form, the sum over the lanes below a lane, is plane_sum(planes, lanes_below(lane)): its
// callers also test the planes for "no lane has any" or store them, so they take ballot_planes once.
template <int PLANES> __device__ __forceinline__ int ballot_sum(int n) { return plane_sum(ballot_planes<PLANES>(n)); }

}  // namespace seunet
