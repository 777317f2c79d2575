// Soft skeleton, soft clDice loss (Shit et al., CVPR 2021) and the hard clDice counts, gfx950.  Definition: tests/cldice_oracle.py.
//
//   erode(x)  = min over the 7-point cross, outside the volume +inf      dilate(x) = max over the 3x3x3 box, outside -inf
//   E_0 = x, E_{j+1} = erode(E_j);  O_j = dilate(E_{j+1});  d_j = relu(E_j - O_j)                  j = 0 .. iters
//   S_0 = d_0;  S_j = S_{j-1} + relu(d_j - S_{j-1} d_j)                                            j = 1 .. iters
//
// Forward: one stencil launch per iteration.  A workgroup stages its tile of E_j with a halo of 2 in LDS, erodes it over the
// tile plus a halo of 1 into a second LDS array, dilates that over the tile, and writes E_{j+1}, S_j and -- when a gradient is
// wanted -- d_j and one byte per voxel: which of the 7 cross voxels gave E_{j+1} (bits 0-2: the first minimum in the order
// d-1, d, d+1, h-1, h+1, w-1, w+1) and which of the 27 box voxels gave O_j (bits 3-7: the first maximum in raster order).
// Everything is a selection or a single float32 add, subtract or multiply; the file is built with -ffp-contract=off, so S is
// the float32 oracle's bit for bit.
//
// Backward: a pointwise pass runs the S recursion backwards (a_j = dL/dd_j, masked), then one stencil launch per iteration in
// GATHER form: every voxel adds, in a fixed order, what the neighbours whose recorded choice points at it pass on.  No float
// atomics anywhere: the results are the same bits from run to run.
//
// Every leading axis is a volume of its own: tiles never span two volumes, and the halo outside a volume is +-inf (forward) or
// "no choice points here" (backward), never the neighbouring volume's voxels.
#include "volume.h"
#include <cmath>

namespace seunet {

namespace {

constexpr int TZ = 4, TY = 8, TX = 64;            // voxels of a tile: 256 threads, two 16-byte quads each
constexpr int HX = 4;                             // the x halo is staged as whole quads: rows of LDS start at x0 - 4
constexpr int AX = TX + 2 * HX;                   // floats per LDS row (288 bytes: rows stay 16-byte aligned)
constexpr int AZ = TZ + 4, AY = TY + 4;           // halo 2
constexpr int BZ = TZ + 2, BY = TY + 2;           // halo 1
constexpr int QUADS = AX / 4;
constexpr unsigned char NO_CHOICE = 0xFF;         // bits 0-2 = 7 and bits 3-7 = 31: matches no cross and no box position

struct Tile { long long base; int z0, y0, x0; };  // base: offset of the tile's volume

__device__ __forceinline__ Tile tile_of(int n0, int n1, int n2) {
  const int tx = (n2 + TX - 1) / TX, ty = (n1 + TY - 1) / TY, tz = (n0 + TZ - 1) / TZ;
  long long b = blockIdx.x;
  Tile t;
  t.x0 = (int)(b % tx) * TX; b /= tx;
  t.y0 = (int)(b % ty) * TY; b /= ty;
  t.z0 = (int)(b % tz) * TZ; b /= tz;
  t.base = b * ((long long)n0 * n1 * n2);
  return t;
}

// LDS[(lz * ny + ly) * AX + lx] = src[z0 - h + lz][y0 - h + ly][x0 - HX + lx], `fill` outside the volume; ny = TY + 2h rows of
// nz = TZ + 2h planes.  VEC: n2 is a multiple of 4 and src is 16-byte aligned, so a quad is inside or outside as a whole.
template <bool VEC>
__device__ __forceinline__ void stage(float* lds, const float* __restrict__ src, float fill, int h, Tile t, int n0, int n1, int n2) {
  const int nz = TZ + 2 * h, ny = TY + 2 * h;
  for (int i = threadIdx.x; i < nz * ny * QUADS; i += 256) {
    const int q = i % QUADS, row = i / QUADS, ly = row % ny, lz = row / ny;
    const int gz = t.z0 - h + lz, gy = t.y0 - h + ly, gx = t.x0 - HX + 4 * q;
    float4 v = make_float4(fill, fill, fill, fill);
    if (gz >= 0 && gz < n0 && gy >= 0 && gy < n1 && src != nullptr) {
      const float* r = src + t.base + ((long long)gz * n1 + gy) * n2;
      if (VEC) {
        if (gx >= 0 && gx < n2) v = *reinterpret_cast<const float4*>(r + gx);
      } else {
        if (gx >= 0 && gx < n2) v.x = r[gx];
        if (gx + 1 >= 0 && gx + 1 < n2) v.y = r[gx + 1];
        if (gx + 2 >= 0 && gx + 2 < n2) v.z = r[gx + 2];
        if (gx + 3 >= 0 && gx + 3 < n2) v.w = r[gx + 3];
      }
    }
    *reinterpret_cast<float4*>(lds + row * AX + 4 * q) = v;
  }
}

template <bool VEC>
__device__ __forceinline__ void stage_bytes(unsigned char* lds, const unsigned char* __restrict__ src, int h, Tile t, int n0, int n1, int n2) {
  const int nz = TZ + 2 * h, ny = TY + 2 * h;
  for (int i = threadIdx.x; i < nz * ny * QUADS; i += 256) {
    const int q = i % QUADS, row = i / QUADS, ly = row % ny, lz = row / ny;
    const int gz = t.z0 - h + lz, gy = t.y0 - h + ly, gx = t.x0 - HX + 4 * q;
    uchar4 v = make_uchar4(NO_CHOICE, NO_CHOICE, NO_CHOICE, NO_CHOICE);
    if (gz >= 0 && gz < n0 && gy >= 0 && gy < n1) {
      const unsigned char* r = src + t.base + ((long long)gz * n1 + gy) * n2;
      if (VEC) {
        if (gx >= 0 && gx < n2) v = *reinterpret_cast<const uchar4*>(r + gx);
      } else {
        if (gx >= 0 && gx < n2) v.x = r[gx];
        if (gx + 1 >= 0 && gx + 1 < n2) v.y = r[gx + 1];
        if (gx + 2 >= 0 && gx + 2 < n2) v.z = r[gx + 2];
        if (gx + 3 >= 0 && gx + 3 < n2) v.w = r[gx + 3];
      }
    }
    *reinterpret_cast<uchar4*>(lds + row * AX + 4 * q) = v;
  }
}

// the cross of `a` (row stride AX, plane stride ps) around index c: its minimum and which position gave it first
__device__ __forceinline__ float erode_at(const float* a, int c, int ps, int& code) {
  float m = a[c - ps], v;
  code = 0;
  v = a[c];      if (v < m) { m = v; code = 1; }
  v = a[c + ps]; if (v < m) { m = v; code = 2; }
  v = a[c - AX]; if (v < m) { m = v; code = 3; }
  v = a[c + AX]; if (v < m) { m = v; code = 4; }
  v = a[c - 1];  if (v < m) { m = v; code = 5; }
  v = a[c + 1];  if (v < m) { m = v; code = 6; }
  return m;
}

// ---- forward: one iteration ------------------------------------------------------------------------------------------------
// e_in = E_j; writes E_{j+1} (e_out, optional), S_j (s_out; s_prev = S_{j-1}, null at j = 0; may alias s_out), d_j and the
// choice bytes (optional).
template <bool VEC>
__global__ void __launch_bounds__(256)
cldice_fwd_kernel(const float* __restrict__ e_in, float* __restrict__ e_out, const float* s_prev, float* s_out,
                  float* __restrict__ d_out, unsigned char* __restrict__ code_out, int n0, int n1, int n2) {
  __shared__ __attribute__((aligned(16))) float A[AZ * AY * AX];   // E_j, halo 2, +inf outside the volume
  __shared__ __attribute__((aligned(16))) float B[BZ * BY * AX];   // E_{j+1}, halo 1, -inf outside the volume
  const Tile t = tile_of(n0, n1, n2);
  stage<VEC>(A, e_in, INFINITY, 2, t, n0, n1, n2);
  __syncthreads();
  for (int i = threadIdx.x; i < BZ * BY * (TX + 2); i += 256) {
    const int bx = i % (TX + 2), by = (i / (TX + 2)) % BY, bz = i / ((TX + 2) * BY);
    const int gz = t.z0 - 1 + bz, gy = t.y0 - 1 + by, gx = t.x0 - 1 + bx;
    float v = -INFINITY;
    if (gz >= 0 && gz < n0 && gy >= 0 && gy < n1 && gx >= 0 && gx < n2) {
      int code;
      v = erode_at(A, ((bz + 1) * AY + by + 1) * AX + bx + HX - 1, AY * AX, code);
    }
    B[(bz * BY + by) * AX + bx + HX - 1] = v;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < TZ * TY * (TX / 4); q += 256) {
    const int qx = q % (TX / 4), qy = (q / (TX / 4)) % TY, qz = q / ((TX / 4) * TY);
    const int gz = t.z0 + qz, gy = t.y0 + qy, gx = t.x0 + 4 * qx;
    if (gz >= n0 || gy >= n1 || gx >= n2) continue;
    const long long at = t.base + ((long long)gz * n1 + gy) * n2 + gx;
    float sp[4] = {0.f, 0.f, 0.f, 0.f}, en[4], dd[4], ss[4];
    unsigned char cc[4];
    if (s_prev != nullptr) {
      if (VEC) {
        const float4 v = *reinterpret_cast<const float4*>(s_prev + at);
        sp[0] = v.x; sp[1] = v.y; sp[2] = v.z; sp[3] = v.w;
      } else {
        for (int k = 0; k < 4; ++k) if (gx + k < n2) sp[k] = s_prev[at + k];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ca = ((qz + 2) * AY + qy + 2) * AX + 4 * qx + k + HX, cb = ((qz + 1) * BY + qy + 1) * AX + 4 * qx + k + HX;
      int cmin, cmax = 0;
      erode_at(A, ca, AY * AX, cmin);
      float o = B[cb - BY * AX - AX - 1];
      int pos = 0;
#pragma unroll
      for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx, ++pos) {
            const float v = B[cb + dz * BY * AX + dy * AX + dx];
            if (v > o) { o = v; cmax = pos; }
          }
      const float diff = A[ca] - o;
      const float d = diff > 0.f ? diff : 0.f;
      float s = d;
      if (s_prev != nullptr) {
        const float r = d - sp[k] * d;
        s = sp[k] + (r > 0.f ? r : 0.f);
      }
      en[k] = B[cb]; dd[k] = d; ss[k] = s;
      cc[k] = (unsigned char)(cmin | (cmax << 3));
    }
    if (VEC) {
      if (e_out) *reinterpret_cast<float4*>(e_out + at) = make_float4(en[0], en[1], en[2], en[3]);
      *reinterpret_cast<float4*>(s_out + at) = make_float4(ss[0], ss[1], ss[2], ss[3]);
      if (d_out) *reinterpret_cast<float4*>(d_out + at) = make_float4(dd[0], dd[1], dd[2], dd[3]);
      if (code_out) *reinterpret_cast<uchar4*>(code_out + at) = make_uchar4(cc[0], cc[1], cc[2], cc[3]);
    } else {
      for (int k = 0; k < 4; ++k)
        if (gx + k < n2) {
          if (e_out) e_out[at + k] = en[k];
          s_out[at + k] = ss[k];
          if (d_out) d_out[at + k] = dd[k];
          if (code_out) code_out[at + k] = cc[k];
        }
    }
  }
}

// ---- the ratio arithmetic on the four sums (float64) --------------------------------------------------------------------------
//   sums[0] = sum S(p) t   sums[1] = sum S(p)   sums[2] = sum S(t) p   sums[3] = sum S(t)
struct Ratios { double a, b, c, d, value, dl_dtprec, dl_dtsens; };
__device__ __forceinline__ Ratios cldice_ratios(const double* __restrict__ sums, double smooth) {
  Ratios r;
  r.a = sums[0] + smooth; r.b = sums[1] + smooth; r.c = sums[2] + smooth; r.d = sums[3] + smooth;
  const double tprec = r.a / r.b, tsens = r.c / r.d, den = tprec + tsens;
  r.value = 1.0 - 2.0 * tprec * tsens / den;
  r.dl_dtprec = -2.0 * tsens * tsens / (den * den);
  r.dl_dtsens = -2.0 * tprec * tprec / (den * den);
  return r;
}

// value[0] = f32(loss); scal[0] = dL/dtprec, scal[1] = dL/dtsens (optional)
__global__ void cldice_value_kernel(const double* __restrict__ sums, double smooth, float* __restrict__ value, double* __restrict__ scal) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const Ratios r = cldice_ratios(sums, smooth);
  value[0] = (float)r.value;
  if (scal) { scal[0] = r.dl_dtprec; scal[1] = r.dl_dtsens; }
}

// ---- the four sums --------------------------------------------------------------------------------------------------------
// The layout of loss.hip's sums (a grid-stride pass, a fixed butterfly per wave, one partial per workgroup, a second launch that
// adds the partials in a fixed order), but in float64 from the first product on: data parallelism adds the sums of the ranks'
// sub-batches, and a sum formed from float32 partials depends on how the voxels fall on the lanes to 1e-8 relative.
constexpr int SUM_BLOCKS = 1024;
__global__ void __launch_bounds__(256)
cldice_sums_kernel(const float* __restrict__ sp, const float* __restrict__ t, const float* __restrict__ st, const float* __restrict__ p,
                   long long n, double* __restrict__ partial) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  auto add = [&](float a, float b, float c, float d) {
    s[0] += (double)a * (double)b; s[1] += (double)a; s[2] += (double)c * (double)d; s[3] += (double)c;
  };
  const bool vec = (n & 3) == 0 && ((reinterpret_cast<size_t>(sp) | reinterpret_cast<size_t>(t) | reinterpret_cast<size_t>(st) |
                                     reinterpret_cast<size_t>(p)) & 15) == 0;
  if (vec) {
    const long long n4 = n >> 2;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
      const float4 a = reinterpret_cast<const float4*>(sp)[i], b = reinterpret_cast<const float4*>(t)[i];
      const float4 c = reinterpret_cast<const float4*>(st)[i], d = reinterpret_cast<const float4*>(p)[i];
      add(a.x, b.x, c.x, d.x); add(a.y, b.y, c.y, d.y); add(a.z, b.z, c.z, d.z); add(a.w, b.w, c.w, d.w);
    }
  } else {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) add(sp[i], t[i], st[i], p[i]);
  }
  __shared__ double red[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double v = wave_sum(s[k]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    partial[blockIdx.x * 4 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// one wave per sum: lane l adds the partials l, l + 64, ..., then the fixed-order butterfly
__global__ void __launch_bounds__(256)
cldice_sums_final_kernel(const double* __restrict__ partial, double* __restrict__ sums) {
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double s = 0.0;
  for (int b = lane; b < SUM_BLOCKS; b += 64) s += partial[b * 4 + k];
  s = wave_sum(s);
  if (lane == 0) sums[k] = s;
}

// ---- backward, pointwise part: the S recursion run backwards ----------------------------------------------------------------
//   G = g dL/dtprec (t b - a) / b^2;  gS = G
//   j = iters .. 1: m = [d_j - S_{j-1} d_j > 0];  a_j = gS m (1 - S_{j-1});  gS = gS - gS m d_j          a_0 = gS [d_0 > 0]
// (m implies d_j > 0, so a_j already carries the relu mask of d_j = relu(E_j - O_j).)  d, s, a: chains of n-voxel volumes.
__global__ void __launch_bounds__(256)
cldice_bwd_chain_kernel(const float* __restrict__ t, const float* __restrict__ d, const float* __restrict__ s, float* __restrict__ a,
                        const double* __restrict__ sums, double smooth, const float* __restrict__ g_dev, long long n, int iters) {
  const Ratios r = cldice_ratios(sums, smooth);
  const double k = (double)g_dev[0] * r.dl_dtprec / (r.b * r.b);
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    float gs = (float)(k * ((double)t[i] * r.b - r.a));
    for (int j = iters; j >= 1; --j) {
      const float dj = d[(size_t)j * n + i], sp = s[(size_t)(j - 1) * n + i];
      const bool m = dj - sp * dj > 0.f;
      a[(size_t)j * n + i] = m ? gs * (1.f - sp) : 0.f;
      if (m) gs = gs - gs * dj;
    }
    a[i] = d[i] > 0.f ? gs : 0.f;
  }
}

// ---- backward, stencil part: one iteration, gather form --------------------------------------------------------------------
//   gE'(q) = gE(q) - sum of a_j(v) over the box voxels v of q whose arg-max is q        (dilate transposed, of -a_j)
//   out(r) = a_j(r) + sum of gE'(q) over the cross voxels q of r whose arg-min is r     (erode transposed)
// g_in = gE (null: zero, the first launch).  The last launch (st != null) adds the tsens term: out += g dL/dtsens S(t) / d.
template <bool VEC>
__global__ void __launch_bounds__(256)
cldice_bwd_kernel(const float* __restrict__ a, const unsigned char* __restrict__ code, const float* __restrict__ g_in,
                  float* __restrict__ g_out, const float* __restrict__ st, const double* __restrict__ sums, double smooth,
                  const float* __restrict__ g_dev, int n0, int n1, int n2) {
  __shared__ __attribute__((aligned(16))) float A[AZ * AY * AX];            // a_j, halo 2, 0 outside the volume
  __shared__ __attribute__((aligned(16))) unsigned char C[AZ * AY * AX];    // choices, halo 2, NO_CHOICE outside
  __shared__ __attribute__((aligned(16))) float B[BZ * BY * AX];            // gE, then gE', halo 1, 0 outside
  const Tile t = tile_of(n0, n1, n2);
  stage<VEC>(A, a, 0.f, 2, t, n0, n1, n2);
  stage_bytes<VEC>(C, code, 2, t, n0, n1, n2);
  stage<VEC>(B, g_in, 0.f, 1, t, n0, n1, n2);
  __syncthreads();
  for (int i = threadIdx.x; i < BZ * BY * (TX + 2); i += 256) {
    const int bx = i % (TX + 2), by = (i / (TX + 2)) % BY, bz = i / ((TX + 2) * BY);
    const int ca = ((bz + 1) * AY + by + 1) * AX + bx + HX - 1, cb = (bz * BY + by) * AX + bx + HX - 1;
    if (C[ca] == NO_CHOICE) continue;                       // outside the volume: B stays 0 and nothing points there
    float g = B[cb];
    int pos = 0;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx, ++pos) {
          const int v = ca + dz * AY * AX + dy * AX + dx;
          if ((C[v] >> 3) == 26 - pos) g = g - A[v];        // v = q + offset(pos) chose q: its own offset is the opposite one
        }
    B[cb] = g;
  }
  __syncthreads();
  float tail = 0.f;
  if (st != nullptr) {
    const Ratios r = cldice_ratios(sums, smooth);
    tail = (float)((double)g_dev[0] * r.dl_dtsens / r.d);
  }
  for (int q = threadIdx.x; q < TZ * TY * (TX / 4); q += 256) {
    const int qx = q % (TX / 4), qy = (q / (TX / 4)) % TY, qz = q / ((TX / 4) * TY);
    const int gz = t.z0 + qz, gy = t.y0 + qy, gx = t.x0 + 4 * qx;
    if (gz >= n0 || gy >= n1 || gx >= n2) continue;
    const long long at = t.base + ((long long)gz * n1 + gy) * n2 + gx;
    float out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ca = ((qz + 2) * AY + qy + 2) * AX + 4 * qx + k + HX, cb = ((qz + 1) * BY + qy + 1) * AX + 4 * qx + k + HX;
      float g = A[ca];
      // q = r + offset(c) chose r when its code is the opposite position: 0 <-> 2, 1 <-> 1, 3 <-> 4, 5 <-> 6
      if ((C[ca - AY * AX] & 7) == 2) g += B[cb - BY * AX];
      if ((C[ca] & 7) == 1) g += B[cb];
      if ((C[ca + AY * AX] & 7) == 0) g += B[cb + BY * AX];
      if ((C[ca - AX] & 7) == 4) g += B[cb - AX];
      if ((C[ca + AX] & 7) == 3) g += B[cb + AX];
      if ((C[ca - 1] & 7) == 6) g += B[cb - 1];
      if ((C[ca + 1] & 7) == 5) g += B[cb + 1];
      out[k] = g;
    }
    if (VEC) {
      if (st != nullptr) {
        const float4 v = *reinterpret_cast<const float4*>(st + at);
        out[0] = out[0] + tail * v.x; out[1] = out[1] + tail * v.y; out[2] = out[2] + tail * v.z; out[3] = out[3] + tail * v.w;
      }
      *reinterpret_cast<float4*>(g_out + at) = make_float4(out[0], out[1], out[2], out[3]);
    } else {
      for (int k = 0; k < 4; ++k)
        if (gx + k < n2) g_out[at + k] = st != nullptr ? out[k] + tail * st[at + k] : out[k];
    }
  }
}

// ---- hard clDice: the four counts of one pass -------------------------------------------------------------------------------
//   counts[0] = |S_P and V_L|   counts[1] = |S_P|   counts[2] = |S_L and V_P|   counts[3] = |S_L|       (masks: non-zero = 1)
__global__ void __launch_bounds__(256)
cldice_counts_kernel(const unsigned char* __restrict__ sp, const unsigned char* __restrict__ vl, const unsigned char* __restrict__ sl,
                     const unsigned char* __restrict__ vp, long long n, u64* __restrict__ counts) {
  unsigned c[4] = {0, 0, 0, 0};
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const bool a = sp[i] != 0, b = sl[i] != 0;
    c[0] += a && vl[i] != 0; c[1] += a; c[2] += b && vp[i] != 0; c[3] += b;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int v = wave_sum((int)c[k]);
    if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(&counts[k], (u64)v);      // integer adds: exact in any order
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

int cldice_check(const char* what, long long volumes, int n0, int n1, int n2, int iters, long long* tiles) {
  SEUNET_CHECK(volumes >= 1 && n0 >= 1 && n1 >= 1 && n2 >= 1, "%s: empty shape (%lld volumes of (%d, %d, %d))", what, volumes, n0, n1, n2);
  SEUNET_CHECK(iters >= 0 && iters <= kCldiceMaxIters, "%s: iters=%d (0..%d)", what, iters, kCldiceMaxIters);
  const long long per = (long long)((n0 + TZ - 1) / TZ) * ((n1 + TY - 1) / TY) * ((n2 + TX - 1) / TX);
  SEUNET_CHECK((long long)n0 * n1 * n2 < (1ll << 31) / volumes && per < (1ll << 31) / volumes,
               "%s: %lld volumes of (%d, %d, %d): fewer than 2^31 voxels in all supported", what, volumes, n0, n1, n2);
  *tiles = per * volumes;
  return 0;
}

}  // namespace

size_t cldice_workspace_bytes(long long volumes, int n0, int n1, int n2, int iters, bool save) {
  WsCarver c(nullptr);
  cldice_ws(c, volumes, n0, n1, n2, iters, save);
  return c.bytes();
}
int cldice_partial_doubles() { return SUM_BLOCKS * 4; }

int launch_soft_skeleton(const float* x, long long volumes, int n0, int n1, int n2, int iters, float* out, bool save, void* workspace,
                         size_t ws_bytes, hipStream_t s) {
  long long tiles;
  if (int e = cldice_check("soft_skeleton", volumes, n0, n1, n2, iters, &tiles)) return e;
  SEUNET_CHECK(x && out && workspace, "soft_skeleton: null argument");
  SEUNET_CHECK(ws_bytes >= cldice_workspace_bytes(volumes, n0, n1, n2, iters, save), "soft_skeleton: workspace too small");
  WsCarver c(workspace);
  const CldiceWs w = cldice_ws(c, volumes, n0, n1, n2, iters, save);
  const size_t n = (size_t)volumes * n0 * n1 * n2;
  const bool vec = (n2 & 3) == 0 && aligned16(x) && aligned16(out) && aligned16(workspace);
  for (int j = 0; j <= iters; ++j) {
    const float* e_in = j == 0 ? x : (j & 1 ? w.e0 : w.e1);
    float* e_out = j == iters ? nullptr : (j & 1 ? w.e1 : w.e0);
    // S_j: saved as a chain when a gradient is wanted (the last one is `out`), else updated in place in `out` (pointwise)
    const float* s_prev = j == 0 ? nullptr : (save ? w.s + (size_t)(j - 1) * n : out);
    float* s_out = (save && j < iters) ? w.s + (size_t)j * n : out;
    float* d_out = save ? w.d + (size_t)j * n : nullptr;
    unsigned char* code_out = save ? w.code + (size_t)j * n : nullptr;
    if (vec) cldice_fwd_kernel<true><<<(unsigned)tiles, 256, 0, s>>>(e_in, e_out, s_prev, s_out, d_out, code_out, n0, n1, n2);
    else cldice_fwd_kernel<false><<<(unsigned)tiles, 256, 0, s>>>(e_in, e_out, s_prev, s_out, d_out, code_out, n0, n1, n2);
  }
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_cldice_sums(const float* sp, const float* t, const float* st, const float* p, long long n, double* partial, double* sums,
                       hipStream_t s) {
  SEUNET_CHECK(sp && t && st && p && partial && sums && n >= 1, "cldice_sums: bad argument");
  cldice_sums_kernel<<<SUM_BLOCKS, 256, 0, s>>>(sp, t, st, p, n, partial);
  cldice_sums_final_kernel<<<1, 256, 0, s>>>(partial, sums);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_cldice_value(const double* sums, double smooth, float* value, double* scal, hipStream_t s) {
  SEUNET_CHECK(sums && value, "cldice_value: null argument");
  cldice_value_kernel<<<1, 64, 0, s>>>(sums, smooth, value, scal);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_cldice_backward(const float* t, const float* st, const double* sums, double smooth, const float* g_dev, long long volumes,
                           int n0, int n1, int n2, int iters, float* grad, void* workspace, size_t ws_bytes, hipStream_t s) {
  long long tiles;
  if (int e = cldice_check("cldice_backward", volumes, n0, n1, n2, iters, &tiles)) return e;
  SEUNET_CHECK(t && st && sums && g_dev && grad && workspace, "cldice_backward: null argument");
  SEUNET_CHECK(ws_bytes >= cldice_workspace_bytes(volumes, n0, n1, n2, iters, true),
               "cldice_backward: the workspace is not the one a saving forward of this shape and iters filled");
  WsCarver c(workspace);
  const CldiceWs w = cldice_ws(c, volumes, n0, n1, n2, iters, true);
  const size_t n = (size_t)volumes * n0 * n1 * n2;
  cldice_bwd_chain_kernel<<<grid_for((long long)n), 256, 0, s>>>(t, w.d, w.s, w.a, sums, smooth, g_dev, (long long)n, iters);
  const bool vec = (n2 & 3) == 0 && aligned16(st) && aligned16(grad) && aligned16(workspace);
  for (int j = iters; j >= 0; --j) {
    // gE ping-pongs through the two E buffers of the forward, which nothing reads after it
    const float* g_in = j == iters ? nullptr : ((iters - j) & 1 ? w.e0 : w.e1);
    float* g_out = j == 0 ? grad : ((iters - j) & 1 ? w.e1 : w.e0);
    const float* tail = j == 0 ? st : nullptr;
    if (vec) cldice_bwd_kernel<true><<<(unsigned)tiles, 256, 0, s>>>(w.a + (size_t)j * n, w.code + (size_t)j * n, g_in, g_out, tail, sums, smooth, g_dev, n0, n1, n2);
    else cldice_bwd_kernel<false><<<(unsigned)tiles, 256, 0, s>>>(w.a + (size_t)j * n, w.code + (size_t)j * n, g_in, g_out, tail, sums, smooth, g_dev, n0, n1, n2);
  }
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_cldice_counts(const unsigned char* sp, const unsigned char* vl, const unsigned char* sl, const unsigned char* vp, long long n,
                         unsigned long long* counts, hipStream_t s) {
  SEUNET_CHECK(sp && vl && sl && vp && counts && n >= 1, "cldice_counts: bad argument");
  SEUNET_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(u64), s));
  cldice_counts_kernel<<<grid_for(n), 256, 0, s>>>(sp, vl, sl, vp, n, counts);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
