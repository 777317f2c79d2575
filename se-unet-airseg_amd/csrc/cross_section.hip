// Airway cross-sections on the device: at every labelled skeleton voxel the lumen section perpendicular to the centreline, as its
// sample count, five integer moments and the samples on the grid's rim.
//
// The reference measures nothing of the kind; the definition is include/seunet_hip.h (seunet_cross_section_emit), restated
// operation by operation in plain numpy by tests/cross_section_oracle.py, and every column equals that oracle bit for bit, the
// float64 tangents included.
//
//   count    one thread per voxel marks the labelled skeleton voxels (skeleton != 0, 1 <= parsing <= num); a wave's ballot is the
//            64-voxel word of the point mask and its popcount the word's count; run_scan (bitvol.h) numbers the points in raster
//            order without atomics.  The host reads the total and the label status once.
//   emit     one thread per word writes the linear index of each of its points at the position the scan gives it.  Then one wave
//            per point, grid-stride, with no launch, pass or synchronise per point or per label:
//            tangent  the lanes stride over the (2W + 1)^3 cells around the point, read `skeleton` and, where it is set, `parsing`;
//                     ten integer sums go through settled butterflies, after which every lane holds them and does the same float64
//                     arithmetic (wave-uniform: no broadcast is needed and no lane waits for another).
//            section  lane r owns row j = r - 31 of the 63 x 63 sample plane as one 64-bit word, bit i + 31 = column i; lane 63 and
//                     bit 63 stay 0 and are the grid's border.  Each lane forms its 63 sample voxels, seven gathers of `parsing` in
//                     flight at a time.  The flood fill from (0, 0) is f |= inside & (f << 1 | f >> 1 | up | down) with `up` /
//                     `down` the neighbouring lanes' words through settled one-lane shuffles, repeated until a ballot says no lane
//                     changed; the fixed point is unique, so the iteration order shows in no result.  Counts and moments are
//                     popcounts of f under the six index-bit masks, summed over the wave by settled butterflies.
// No LDS, no atomics, no floating-point reduction: nothing depends on the launch shape.
#include "volume.h"
#include "cross_basis.h"
#include <cmath>

// the tangent, the basis and the sample positions are the oracle's float64 arithmetic operation by operation
#pragma clang fp contract(off)

namespace seunet {

namespace {

constexpr int kHalf = 31;                 // the sample plane is (2 kHalf + 1)^2: one 64-bit word per row, one row per lane
constexpr int kSide = 2 * kHalf + 1;
constexpr int kSectionBlocks = 2048;      // workgroups of the section pass: 4 waves each, 8192 points per grid sweep
constexpr int kGathers = 7;               // sample voxels a lane has in flight; kSide = 9 x 7
constexpr int kPowerSteps = 6;            // squarings of the scatter matrix: its 64th power
static_assert(kSide % kGathers == 0, "a row is a whole number of gather groups");

// bits of a word whose index has bit k set
__host__ __device__ constexpr u64 index_bit_mask(int k) {
  constexpr u64 m[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull,
                        0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
  return m[k];
}

// ---- count -------------------------------------------------------------------------------------------------------------------
// one thread per voxel; word w of the point mask = voxels 64 w .. 64 w + 63 in raster order = one wave
__global__ void __launch_bounds__(256)
cross_mark_kernel(const int* __restrict__ parsing, const unsigned char* __restrict__ skel, long long n, int num, u64* __restrict__ bits,
                  unsigned* __restrict__ cnt, CrossRec* __restrict__ rec) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  bool set = false;
  if (i < n) {
    int a = parsing[i];
    if (a < 0 || a > num) { rec->status = 1; a = 0; }
    set = a > 0 && skel[i] != 0;
  }
  const u64 m = __ballot(set);
  if ((threadIdx.x & 63) == 0 && i < n) {
    bits[i >> 6] = m;
    cnt[i >> 6] = (unsigned)__popcll(m);
  }
}

// ---- emit --------------------------------------------------------------------------------------------------------------------
// one thread per word: the linear index of every point at its raster-order position
__global__ void __launch_bounds__(256)
cross_points_kernel(const u64* __restrict__ bits, const unsigned* __restrict__ cnt, const unsigned* __restrict__ blk, long long nwords,
                    long long m, int* __restrict__ lin) {
  const long long w = blockIdx.x * 256ll + threadIdx.x;
  if (w >= nwords) return;
  u64 b = bits[w];
  long long pos = (long long)cnt[w] + blk[w / kScanBlock];
  while (b) {
    if (pos < m) lin[pos] = (int)(w * 64 + __builtin_ctzll(b));      // (pos >= m cannot happen with the total of the count call)
    b &= b - 1;
    ++pos;
  }
}

struct CrossParams {
  int n0, n1, n2, window, same_label;
  double s[3], h;
};

__device__ __forceinline__ double max9(const double (&a)[3][3]) {
  double m = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) m = fmax(m, fabs(a[r][c]));
  return m;
}

// The unit tangent from the ten integer sums of the window; false: invalid (t = 0).  Every lane calls it with the same values.
__device__ __forceinline__ bool cross_tangent(long long n, const long long (&sd)[3], const long long (&sdd)[6], const double (&sp)[3],
                                              double (&t)[3]) {
  t[0] = t[1] = t[2] = 0.0;
  if (n < 3) return false;
  double a[3][3];
  {
    int at = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = r; c < 3; ++c) {                          // sdd: 00, 01, 02, 11, 12, 22
        const long long scatter = n * sdd[at++] - sd[r] * sd[c];
        a[r][c] = a[c][r] = ((double)scatter * sp[r]) * sp[c];
      }
  }
  double top = max9(a);
  if (!(top > 0.0)) return false;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) a[r][c] = a[r][c] / top;
  for (int step = 0; step < kPowerSteps; ++step) {
    double b[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) b[r][c] = (a[r][0] * a[0][c] + a[r][1] * a[1][c]) + a[r][2] * a[2][c];
    top = max9(b);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) a[r][c] = b[r][c] / top;
  }
  double best = -1.0, col[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < 3; ++c) {                              // the column of largest squared length, the lowest on a tie
    const double len2 = (a[0][c] * a[0][c] + a[1][c] * a[1][c]) + a[2][c] * a[2][c];
    if (len2 > best) {
      best = len2;
      col[0] = a[0][c]; col[1] = a[1][c]; col[2] = a[2][c];
    }
  }
  const double len = sqrt(best);
#pragma unroll
  for (int q = 0; q < 3; ++q) t[q] = col[q] / len;
  double lead = t[0];                                        // the component of largest magnitude, the lowest on a tie
  if (fabs(t[1]) > fabs(lead)) lead = t[1];
  if (fabs(t[2]) > fabs(lead)) lead = t[2];
  if (lead < 0.0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) t[q] = -t[q];
  }
  return true;
}

// one wave per point, grid-stride.  table: 12 int32 per point (i0, i1, i2, label, support, count, sum i, sum j, sum i^2,
// sum j^2, sum ij, rim); tangent: 3 float64 per point.
__global__ void __launch_bounds__(256)
cross_section_kernel(const int* __restrict__ parsing, const unsigned char* __restrict__ skel, const int* __restrict__ lin, long long m,
                     CrossParams p, double* __restrict__ tangent, int* __restrict__ table) {
  const int lane = threadIdx.x & 63;
  const long long plane = (long long)p.n1 * p.n2;
  const long long waves = gridDim.x * 4ll;
  for (long long q = (blockIdx.x * 256ll + threadIdx.x) >> 6; q < m; q += waves) {      // wave-uniform
    const long long at = lin[q];
    if (at < 0 || at >= (long long)p.n0 * plane) continue;     // (cannot happen with the total of the count call)
    const Vox3 c = vox3(at, p.n1, p.n2);
    const int label = parsing[at];

    // ---- tangent: the ten sums of d = q - p over the label's skeleton voxels of the window
    const int side = 2 * p.window + 1, cells = side * side * side;
    int part[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};           // n, d0, d1, d2, d0 d0, d0 d1, d0 d2, d1 d1, d1 d2, d2 d2
    for (int cell = lane; cell < cells; cell += 64) {
      const int d0 = cell / (side * side) - p.window, d1 = cell / side % side - p.window, d2 = cell % side - p.window;
      const int x0 = c.i0 + d0, x1 = c.i1 + d1, x2 = c.i2 + d2;
      if (x0 < 0 || x0 >= p.n0 || x1 < 0 || x1 >= p.n1 || x2 < 0 || x2 >= p.n2) continue;
      const long long j = at + d0 * plane + (long long)d1 * p.n2 + d2;
      if (skel[j] == 0 || parsing[j] != label) continue;
      part[0] += 1;
      part[1] += d0; part[2] += d1; part[3] += d2;
      part[4] += d0 * d0; part[5] += d0 * d1; part[6] += d0 * d2;
      part[7] += d1 * d1; part[8] += d1 * d2; part[9] += d2 * d2;
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) part[k] = wave_sum(part[k]);
    const long long sd[3] = {part[1], part[2], part[3]};
    const long long sdd[6] = {part[4], part[5], part[6], part[7], part[8], part[9]};
    double t[3];
    const bool valid = cross_tangent(part[0], sd, sdd, p.s, t);      // wave-uniform: every lane holds the same sums

    // ---- section
    int sums[7] = {0, 0, 0, 0, 0, 0, 0};                     // count, sum i, sum j, sum i^2, sum j^2, sum ij, rim
    if (valid) {                                             // (wave-uniform)
      double u[3], v[3];
      cross_basis(t, u, v);
      u64 inside = 0ull;
      if (lane < kSide) {
        const double jh = (double)(lane - kHalf) * p.h;
        const double centre[3] = {(double)c.i0 * p.s[0], (double)c.i1 * p.s[1], (double)c.i2 * p.s[2]};
        const double jv[3] = {jh * v[0], jh * v[1], jh * v[2]};
        const double ext[3] = {(double)p.n0, (double)p.n1, (double)p.n2};
        for (int b0 = 0; b0 < kSide; b0 += kGathers) {
          int got[kGathers];
          bool in[kGathers];
#pragma unroll
          for (int g = 0; g < kGathers; ++g) {               // the loads of a group are issued before the first is used
            const double ih = (double)(b0 + g - kHalf) * p.h;
            double f[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              const double x = (centre[a] + ih * u[a]) + jv[a];
              f[a] = floor(x / p.s[a] + 0.5);
            }
            in[g] = f[0] >= 0.0 && f[0] < ext[0] && f[1] >= 0.0 && f[1] < ext[1] && f[2] >= 0.0 && f[2] < ext[2];
            // a sample outside the volume reads the centre, a legal address
            const long long j = in[g] ? ((long long)f[0] * p.n1 + (long long)f[1]) * p.n2 + (long long)f[2] : at;
            got[g] = parsing[j];
          }
#pragma unroll
          for (int g = 0; g < kGathers; ++g)
            if (in[g] && (p.same_label ? got[g] == label : got[g] != 0)) inside |= 1ull << (b0 + g);
        }
      }
      u64 f = lane == kHalf ? inside & (1ull << kHalf) : 0ull;
      for (;;) {                                             // wave-uniform: leaves when no lane changed
        const u64 above = dpp_settle(__shfl_up(f, 1, 64)), below = dpp_settle(__shfl_down(f, 1, 64));
        const u64 up = lane > 0 ? above : 0ull, down = lane < 63 ? below : 0ull;
        const u64 next = f | (inside & ((f << 1) | (f >> 1) | up | down));
        const bool changed = next != f;
        f = next;
        if (__ballot(changed) == 0) break;
      }
      // per row: count, sum of the bit index b and of b^2 from popcounts under the index-bit masks; i = b - kHalf, j = lane - kHalf
      const int cnt = __popcll(f);
      int sb = 0, sbb = 0;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int ck = __popcll(f & index_bit_mask(k));
        sb += ck << k;
        sbb += ck << (2 * k);
#pragma unroll
        for (int l = k + 1; l < 6; ++l) sbb += __popcll(f & index_bit_mask(k) & index_bit_mask(l)) << (k + l + 1);
      }
      const int j = lane - kHalf;
      const int si = sb - kHalf * cnt, sii = sbb - 2 * kHalf * sb + kHalf * kHalf * cnt;
      sums[0] = cnt;
      sums[1] = si;
      sums[2] = j * cnt;
      sums[3] = sii;
      sums[4] = j * j * cnt;
      sums[5] = j * si;
      sums[6] = (lane == 0 || lane == kSide - 1) ? cnt : __popcll(f & (1ull | 1ull << (kSide - 1)));
#pragma unroll
      for (int k = 0; k < 7; ++k) sums[k] = wave_sum(sums[k]);
    }
    if (lane == 0) {
      int* row = table + 12 * q;
      row[0] = c.i0; row[1] = c.i1; row[2] = c.i2;
      row[3] = label;
      row[4] = part[0];
#pragma unroll
      for (int k = 0; k < 7; ++k) row[5 + k] = sums[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) tangent[3 * q + k] = t[k];
    }
  }
}

}  // namespace

size_t cross_section_workspace_bytes(int n0, int n1, int n2) { return measured(cross_section_ws, n0, n1, n2); }
int cross_section_sweep_points() { return kSectionBlocks * 4; }

int launch_cross_section_count(const int* parsing, const unsigned char* skeleton, int n0, int n1, int n2, int num, long long* m, int* status,
                               void* workspace, size_t ws_bytes, hipStream_t s) {
  SEUNET_CHECK(parsing && skeleton && m && status && workspace, "cross_section_count: null argument");
  if (int e = volume_check("cross_section_count", n0, n1, n2, 0)) return e;
  SEUNET_CHECK(num >= 0 && num <= label_stats_max_num(), "cross_section_count: num %d: labels 0 .. %d are supported", num,
               label_stats_max_num());
  WsCarver carve(workspace);
  const CrossWs w = cross_section_ws(carve, n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "cross_section_count: workspace too small (%zu bytes, %zu needed)", ws_bytes, carve.bytes());
  const long long n = (long long)n0 * n1 * n2, nwords = (n + 63) / 64;
  SEUNET_HIP(hipMemsetAsync(w.rec, 0, sizeof(CrossRec), s));
  cross_mark_kernel<<<blocks_256(n), 256, 0, s>>>(parsing, skeleton, n, num, w.bits, w.cnt, w.rec);
  if (int e = run_scan(w.cnt, nullptr, nwords, w.blk, nullptr, w.rec->total, s)) return e;
  CrossRec host;                                               // the one synchronisation: the number of points and the status
  SEUNET_HIP(hipMemcpyAsync(&host, w.rec, sizeof(CrossRec), hipMemcpyDeviceToHost, s));
  SEUNET_HIP(hipStreamSynchronize(s));
  *m = (long long)host.total[0];
  *status = host.status;
  return 0;
}

int launch_cross_section_emit(const int* parsing, const unsigned char* skeleton, int n0, int n1, int n2, double s0, double s1, double s2,
                              double step, int window, int same_label, long long m, int* lin, double* tangent, int* table,
                              const void* workspace, size_t ws_bytes, hipStream_t s) {
  SEUNET_CHECK(parsing && skeleton && lin && tangent && table && workspace, "cross_section_emit: null argument");
  if (int e = volume_check("cross_section_emit", n0, n1, n2, 0)) return e;
  SEUNET_CHECK(s0 > 0.0 && s1 > 0.0 && s2 > 0.0 && s0 < HUGE_VAL && s1 < HUGE_VAL && s2 < HUGE_VAL,
               "cross_section_emit: the spacing must be three positive finite numbers, got (%g, %g, %g)", s0, s1, s2);
  SEUNET_CHECK(step > 0.0 && step < HUGE_VAL, "cross_section_emit: the step must be positive and finite, got %g", step);
  SEUNET_CHECK(window >= 1 && window <= 7, "cross_section_emit: window %d: 1 .. 7 are supported", window);
  const long long n = (long long)n0 * n1 * n2, nwords = (n + 63) / 64;
  SEUNET_CHECK(m >= 1 && m <= n, "cross_section_emit: %lld points in a volume of %lld voxels", m, n);
  WsCarver carve(const_cast<void*>(workspace));
  const CrossWs w = cross_section_ws(carve, n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "cross_section_emit: workspace too small (%zu bytes, %zu needed)", ws_bytes, carve.bytes());
  cross_points_kernel<<<blocks_256(nwords), 256, 0, s>>>(w.bits, w.cnt, w.blk, nwords, m, lin);
  const CrossParams p{n0, n1, n2, window, same_label != 0, {s0, s1, s2}, step};
  const unsigned blocks = (unsigned)std::min<long long>((m + 3) / 4, kSectionBlocks);
  cross_section_kernel<<<blocks, 256, 0, s>>>(parsing, skeleton, lin, m, p, tangent, table);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
