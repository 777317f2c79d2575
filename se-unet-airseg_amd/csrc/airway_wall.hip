// Airway wall measurement on the device: at every centreline point 64 rays in the section plane, the CT sampled along each, and
// the wall's inner and outer edge by the full-width-at-half-maximum rule.
//
// The reference measures nothing of the kind; the definition is include/seunet_hip.h (seunet_airway_walls), restated operation by
// operation in plain numpy by tests/airway_wall_oracle.py, and every output equals that oracle bit for bit.
//
// One launch, one wave per point, grid-stride, lane r = ray r:
//   frame    every lane forms u, v (cross_basis.h, the section pass's), the lumen centroid and its own direction e.
//   labels   the lane walks its 64 samples in groups of kLabelGroup nearest-voxel gathers of `parsing`, issued before the first is
//            used, and keeps three 64-bit words: usable, inside, non-zero label.  A lane needs nothing past its first unusable
//            sample or 2 n_search + 2 samples past its first outside sample, so the wave leaves the loop when no lane needs more.
//   profile  groups of kCtGroup samples, their 8 x kCtGroup corner gathers of the CT issued before the first is used; the float32
//            trilinear value goes to LDS as profile[k][lane]: a lane's 64 values cannot be a register array that is indexed
//            dynamically (that is scratch memory), and [k][lane] has the 64 lanes of a wave on 64 consecutive dwords, so no access
//            has a bank conflict.  A lane reads only what it wrote itself: no barrier.
//   rules    each lane runs the definition's scans over its own column.
//   sums     six float64 xor butterflies in the fixed order of the definition; the mask is a ballot.
// No atomics, no workspace, nothing that depends on the launch shape.
#include "volume.h"
#include "cross_basis.h"
#include "wall_table.h"
#include <cmath>

// the frame, the sample positions, the interpolation and the edges are the oracle's arithmetic operation by operation
#pragma clang fp contract(off)

namespace seunet {

namespace {

constexpr int kRays = SEUNET_WALL_RAYS;   // one per lane
constexpr int kSamples = 64;              // per ray: one bit of a 64-bit word each
constexpr int kWallBlocks = 2048;         // workgroups: 4 waves each, 8192 points per grid sweep
constexpr int kLabelGroup = 8;            // label gathers a lane has in flight
constexpr int kCtGroup = 4;               // samples whose eight corner gathers a lane has in flight
static_assert(kRays == 64 && kSamples % kLabelGroup == 0 && kSamples % kCtGroup == 0, "one ray per lane, whole gather groups");

struct WallTable { double d[kRays][2]; };
constexpr WallTable make_wall_table() {
  WallTable t{};
  for (int r = 0; r < kRays; ++r) { t.d[r][0] = kWallDirections[r][0]; t.d[r][1] = kWallDirections[r][1]; }
  return t;
}
__constant__ WallTable d_wall_table = make_wall_table();

struct WallParams {
  int n0, n1, n2, n_search, same_label;
  float min_contrast;
  double s[3], h, dr;
};

__device__ __forceinline__ float ct_value(short v) { return (float)v; }
__device__ __forceinline__ float ct_value(float v) { return v; }

// sample k of a ray: g = x / s per axis and f = floor(g); true when all eight corners f, f + 1 lie in the volume
__device__ __forceinline__ bool wall_sample(const WallParams& p, const double (&o)[3], const double (&e)[3], int k, double (&g)[3],
                                            double (&f)[3]) {
  const double rho = (double)k * p.dr;
  const double top[3] = {(double)(p.n0 - 2), (double)(p.n1 - 2), (double)(p.n2 - 2)};
  bool usable = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double x = o[a] + rho * e[a];
    g[a] = x / p.s[a];
    f[a] = floor(g[a]);
    usable = usable && f[a] >= 0.0 && f[a] <= top[a];
  }
  return usable;
}

// table: 12 int32 per point as seunet_cross_section_emit writes them; tangent: 3 float64 per point
template <typename T>
__global__ void __launch_bounds__(256)
airway_wall_kernel(const T* __restrict__ ct, const int* __restrict__ parsing, long long m, WallParams p, const int* __restrict__ table,
                   const double* __restrict__ tangent, u64* __restrict__ mask, double* __restrict__ sums,
                   unsigned char* __restrict__ codes, double* __restrict__ edges) {
  __shared__ float profile[4][kSamples][kRays];
  const int lane = threadIdx.x & 63;
  float (&P)[kSamples][kRays] = profile[threadIdx.x >> 6];
  const long long plane = (long long)p.n1 * p.n2;
  const long long waves = gridDim.x * 4ll;
  const double dir_c = d_wall_table.d[lane][0], dir_s = d_wall_table.d[lane][1];
  for (long long q = (blockIdx.x * 256ll + threadIdx.x) >> 6; q < m; q += waves) {      // wave-uniform
    const int* row = table + 12 * q;
    const int label = row[3], count = row[5], rim = row[11];
    int code = 6;
    double rho_in = 0.0, rho_out = 0.0;
    float peak = 0.0f;
    if (count != 0 && rim <= 0) {                            // (wave-uniform)
      // ---- frame
      const double t[3] = {tangent[3 * q], tangent[3 * q + 1], tangent[3 * q + 2]};
      double u[3], v[3], o[3], e[3];
      cross_basis(t, u, v);
      const double ci = (double)row[6] / (double)count, cj = (double)row[7] / (double)count;
      const double cih = ci * p.h, cjh = cj * p.h;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        o[a] = ((double)row[a] * p.s[a] + cih * u[a]) + cjh * v[a];
        e[a] = dir_c * u[a] + dir_s * v[a];
      }

      // ---- labels: bit k of usable / inside / nonzero; `need` = the samples this lane can still ask for
      u64 usable = 0ull, inside = 0ull, nonzero = 0ull;
      int need = kSamples, reach = 0;                        // reach: samples evaluated
      for (int k0 = 0; k0 < kSamples; k0 += kLabelGroup) {   // wave-uniform
        int got[kLabelGroup];
        bool ok[kLabelGroup];
#pragma unroll
        for (int j = 0; j < kLabelGroup; ++j) {              // the loads of a group are issued before the first is used
          double g[3], f[3];
          ok[j] = wall_sample(p, o, e, k0 + j, g, f);
          // the nearest voxel of a usable sample lies in the volume; any other sample reads voxel 0, a legal address
          const long long at = ok[j] ? ((long long)floor(g[0] + 0.5) * p.n1 + (long long)floor(g[1] + 0.5)) * p.n2 +
                                           (long long)floor(g[2] + 0.5)
                                     : 0ll;
          got[j] = parsing[at];
        }
#pragma unroll
        for (int j = 0; j < kLabelGroup; ++j) {
          const int k = k0 + j;
          const bool in = ok[j] && (p.same_label ? got[j] == label : got[j] != 0);
          if (ok[j]) usable |= 1ull << k;
          if (ok[j] && got[j] != 0) nonzero |= 1ull << k;
          if (in) inside |= 1ull << k;
          if (need == kSamples && !in) need = !ok[j] || k == 0 ? k : min(kSamples, k + 2 * p.n_search + 2);
        }
        reach = k0 + kLabelGroup;
        if (__all(reach >= need)) break;
      }
      // L: the first unusable sample among those evaluated; what lies past `reach` is past every index the rules can ask for
      const int L = usable == ~0ull ? kSamples : min(reach, (int)__builtin_ctzll(~usable));
      const u64 below_l = L >= 64 ? ~0ull : (1ull << L) - 1ull;
      const u64 outside = ~inside & below_l & ~1ull;
      const bool bounded = L > 0 && (inside & 1ull) != 0ull && outside != 0ull;
      const int kb = bounded ? (int)__builtin_ctzll(outside) : 0;
      const int samples = bounded ? min(L, kb + 2 * p.n_search + 2) : 0;

      // ---- profile: P[k][lane] for k < samples
      for (int k0 = 0; __any(k0 < samples); k0 += kCtGroup) {      // wave-uniform
        float c[kCtGroup][8], w[kCtGroup][3];
#pragma unroll
        for (int j = 0; j < kCtGroup; ++j) {
          double g[3], f[3];
          const bool live = k0 + j < samples && wall_sample(p, o, e, k0 + j, g, f);      // (k < samples <= L: usable)
#pragma unroll
          for (int a = 0; a < 3; ++a) w[j][a] = (float)(g[a] - f[a]);
          // a lane without this sample reads voxel 0 eight times
          const long long at = live ? ((long long)f[0] * p.n1 + (long long)f[1]) * p.n2 + (long long)f[2] : 0ll;
          const long long d0 = live ? plane : 0ll, d1 = live ? (long long)p.n2 : 0ll, d2 = live ? 1ll : 0ll;
#pragma unroll
          for (int b = 0; b < 8; ++b) c[j][b] = ct_value(ct[at + (b >> 2 & 1) * d0 + (b >> 1 & 1) * d1 + (b & 1) * d2]);
        }
#pragma unroll
        for (int j = 0; j < kCtGroup; ++j) {                 // along axis 2, then axis 1, then axis 0; each step a + w (b - a)
          const float c00 = c[j][0] + w[j][2] * (c[j][1] - c[j][0]), c01 = c[j][2] + w[j][2] * (c[j][3] - c[j][2]);
          const float c10 = c[j][4] + w[j][2] * (c[j][5] - c[j][4]), c11 = c[j][6] + w[j][2] * (c[j][7] - c[j][6]);
          const float c0 = c00 + w[j][1] * (c01 - c00), c1 = c10 + w[j][1] * (c11 - c10);
          P[k0 + j][lane] = c0 + w[j][0] * (c1 - c0);
        }
      }

      // ---- rules: the first that fails gives the code
      code = 1;
      if (bounded) {
        const int lo = max(kb - 1, 0), hi = min(kb + p.n_search, L - 1);
        int kp = lo;
        float pp = P[lo][lane];
        for (int k = lo + 1; k <= hi; ++k) {
          const float x = P[k][lane];
          if (x > pp) { pp = x; kp = k; }
        }
        code = 2;
        if (kp + 1 < L && !(kp == hi && P[kp + 1][lane] >= pp)) {
          float pl = pp;
          for (int k = 0; k < kp; ++k) {
            const float x = P[k][lane];
            if (x < pl) pl = x;
          }
          code = 3;
          if (!(pp - pl < p.min_contrast)) {
            const int stop = min(kp + p.n_search, L - 1);
            int ko = kp;
            float po = pp;
            while (ko < stop) {
              const float x = P[ko + 1][lane];
              if (!(x <= po)) break;
              po = x;
              ++ko;
            }
            const u64 walked = ko >= kb ? (~0ull >> (63 - ko)) & (~0ull << kb) : 0ull;      // bits kb .. ko
            code = 4;
            if ((nonzero & walked) == 0ull) {
              code = 5;
              if (!(pp - po < p.min_contrast)) {
                code = 0;
                peak = pp;
                const float h_in = 0.5f * (pl + pp);
                int ki = max(kp - 1, 0);                     // (a measured ray has k_p >= 1: P_p exceeds P_l)
                while (ki > 0 && !(P[ki][lane] <= h_in)) --ki;
                const double a_in = (double)P[ki][lane];
                rho_in = ((double)ki + ((double)h_in - a_in) / ((double)P[ki + 1][lane] - a_in)) * p.dr;
                const float h_out = 0.5f * (pp + po);
                int ke = kp;
                while (ke < ko - 1 && !(P[ke + 1][lane] <= h_out)) ++ke;
                const double a_out = (double)P[ke][lane];
                rho_out = ((double)ke + (a_out - (double)h_out) / (a_out - (double)P[ke + 1][lane])) * p.dr;
              }
            }
          }
        }
      }
    }

    // ---- per point: the mask and the six sums by the xor butterfly T_{l+1}[r] = T_l[r] + T_l[r ^ (1 << l)]
    const u64 measured = __ballot(code == 0);
    double total[6] = {rho_in, rho_out, rho_in * rho_in, rho_out * rho_out, rho_out - rho_in, (double)peak};
#pragma unroll
    for (int l = 0; l < 6; ++l)
#pragma unroll
      for (int k = 0; k < 6; ++k) total[k] = total[k] + shfl_xor_settled(total[k], 1 << l);
    if (lane == 0) {
      mask[q] = measured;
#pragma unroll
      for (int k = 0; k < 6; ++k) sums[6 * q + k] = total[k];
    }
    if (codes) codes[kRays * q + lane] = (unsigned char)code;
    if (edges) {
      edges[2 * (kRays * q + lane)] = rho_in;
      edges[2 * (kRays * q + lane) + 1] = rho_out;
    }
  }
}

}  // namespace

int airway_wall_rays() { return kRays; }
int airway_wall_samples() { return kSamples; }
int airway_wall_sweep_points() { return kWallBlocks * 4; }
void airway_wall_directions(double* out) {
  for (int r = 0; r < kRays; ++r) {
    out[2 * r] = kWallDirections[r][0];
    out[2 * r + 1] = kWallDirections[r][1];
  }
}

int launch_airway_walls(const void* ct, int ct_dtype, const int* parsing, int n0, int n1, int n2, double s0, double s1, double s2,
                        double step, double ray_step, int n_search, float min_contrast, int same_label, long long m, const int* table,
                        const double* tangent, unsigned long long* mask, double* sums, unsigned char* codes, double* edges,
                        hipStream_t s) {
  SEUNET_CHECK(ct && parsing && table && tangent && mask && sums, "airway_walls: null argument");
  SEUNET_CHECK(ct_dtype == 0 || ct_dtype == 1, "airway_walls: ct_dtype %d: SEUNET_IMG_I16 and SEUNET_IMG_F32 are supported", ct_dtype);
  if (int e = volume_check("airway_walls", n0, n1, n2, 0)) return e;
  SEUNET_CHECK(s0 > 0.0 && s1 > 0.0 && s2 > 0.0 && s0 < HUGE_VAL && s1 < HUGE_VAL && s2 < HUGE_VAL,
               "airway_walls: the spacing must be three positive finite numbers, got (%g, %g, %g)", s0, s1, s2);
  SEUNET_CHECK(step > 0.0 && step < HUGE_VAL, "airway_walls: the section step must be positive and finite, got %g", step);
  SEUNET_CHECK(ray_step > 0.0 && ray_step < HUGE_VAL, "airway_walls: the ray step must be positive and finite, got %g", ray_step);
  SEUNET_CHECK(n_search >= 1 && n_search <= 31, "airway_walls: n_search %d: 1 .. 31 are supported", n_search);
  SEUNET_CHECK(min_contrast > 0.0f && min_contrast < HUGE_VALF, "airway_walls: min_contrast must be positive and finite, got %g",
               (double)min_contrast);
  SEUNET_CHECK(m >= 1, "airway_walls: %lld points", m);
  const WallParams p{n0, n1, n2, n_search, same_label != 0, min_contrast, {s0, s1, s2}, step, ray_step};
  const unsigned blocks = (unsigned)std::min<long long>((m + 3) / 4, kWallBlocks);
  if (ct_dtype == 0)
    airway_wall_kernel<<<blocks, 256, 0, s>>>((const short*)ct, parsing, m, p, table, tangent, (u64*)mask, sums, codes, edges);
  else
    airway_wall_kernel<<<blocks, 256, 0, s>>>((const float*)ct, parsing, m, p, table, tangent, (u64*)mask, sums, codes, edges);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
