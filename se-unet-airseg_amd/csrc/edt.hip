// Stage-2 / stage-3 preparation on the device: the exact Euclidean distance transform with its feature transform, the
// hard-mining candidate masks, the LIB weight map and the break weight (DESIGN.md "Preparation").
//
// Reference (CPU, scipy / skimage / cc3d behind it):
//   data.py:304-306, 455-458   dis = distance_transform_edt(label); loc_small = where(dis * skeleton < 2);
//                              loc_skeleton = where(skeleton * (1 - pred))           (every stage-2/3 __getitem__)
//   lib_weight.py:12-17, 36-53 7x7x7 box filter (mode 'mirror') / 343, 0 -> 1, -log10, * label, float16
//   weight_br.py:113-177       save_weight_break: two EDTs with indices, 26-connected components, a 3x3x3 neighbour count,
//                              a dilation shell and a float16 weight chain
//
// EDT.  scipy's feature transform (ni_morphology.c) is separable: a pass along axis 0, then axis 1, then axis 2, each a 1-D
// Voronoi step on every line using the features of the previous passes.  One lane walks one line and keeps scipy's order:
//   build: scan the line's sites (voxels with a feature) in order; a stack of sites; with the top two entries (offsets uR,
//          vR off the line, positions g1 < g2) and the new site (wR, position p): a = g2 - g1, b = p - g2, c = a + b, pop while
//          c*vR - b*uR - a*wR - a*b*c > 0, then push;
//   query: walk the positions in order and advance to the next stack site only while it is STRICTLY closer (a tie keeps
//          the earlier site).
// Pass 0 is "nearest site along the line, ties to the lower coordinate".  Every quantity is an integer below 2^53 and the
// arithmetic is int64, so the features are scipy's, ties included.  Between passes features are int16 (extents <= 32767);
// the stack of a line lives in a volume-shaped workspace at the line's own voxels (entry k at position k), so lanes of a
// wave touch the same lines of memory as their input reads.  Distances are sqrt of the integer in double (correctly rounded,
// checked over every integer up to 3 * 1024^2 by tests/test_prep_gpu.py).
//
// Integer / index work and IEEE-rounded float chains in the reference's order: results are bit-identical to the reference
// (tests/test_prep_gpu.py against tests/golden/prep_known.npz).
#include "volume.h"
#include <algorithm>

// numpy does not contract a * b + c into a fused multiply-add; hipcc does by default
#pragma clang fp contract(off)

namespace seunet {

// ---- exact EDT / feature transform ----------------------------------------------------------------------------------

// pass 0: one lane per (i1, i2) column; f0 = coordinate along axis 0 of the nearest site (-1: none), ties to the lower one.
// INVERT = false: sites are the zero voxels (distance_transform_edt(vol)); true: the non-zero ones (EDT of 1 - vol).
template <bool INVERT>
__global__ void __launch_bounds__(256)
edt_pass0_kernel(const unsigned char* __restrict__ vol, int n0, long long plane, short* __restrict__ f0, int* __restrict__ status) {
  const long long c = blockIdx.x * 256ll + threadIdx.x;
  if (c >= plane) return;
  int last = -1;
  for (int i = 0; i < n0; ++i) {
    if ((vol[i * plane + c] != 0) == INVERT) last = i;
    f0[i * plane + c] = (short)last;
  }
  if (last >= 0 && status) *status = 0;      // some site exists (the launcher preset 1)
  int next = -1;
  for (int i = n0 - 1; i >= 0; --i) {
    const int p = f0[i * plane + c];
    if (p == i) next = i;
    else if (next >= 0 && (p < 0 || next - i < i - p)) f0[i * plane + c] = (short)next;
  }
}

// EdtOut (what the last pass writes, each part optional) and the workspace layout EdtWs: volume.h

// pass D (1 or 2) along axis D.  in0 / in1: features along axes 0 / 1 of the previous passes (in1 for D == 2 only).
// D == 1 writes out0 / out1 (features along axes 0 / 1); D == 2 writes the final outputs.
// spos / sr: the stack of each line, volume-shaped (entry k at the voxel of position k).
template <int D>
__global__ void __launch_bounds__(256)
edt_pass_kernel(const short* __restrict__ in0, const short* __restrict__ in1, int n0, int n1, int n2,
                short* __restrict__ spos, int* __restrict__ sr, short* __restrict__ out0, short* __restrict__ out1, EdtOut o) {
  const long long line = blockIdx.x * 256ll + threadIdx.x;
  long long base, stride, nlines;
  int len, c0, c1;
  if (D == 1) {            // line (i0, i2)
    nlines = (long long)n0 * n2;
    if (line >= nlines) return;
    c0 = (int)(line / n2);
    c1 = 0;
    const int i2 = (int)(line % n2);
    base = (long long)c0 * n1 * n2 + i2;
    stride = n2;
    len = n1;
  } else {                 // line (i0, i1)
    nlines = (long long)n0 * n1;
    if (line >= nlines) return;
    c0 = (int)(line / n1);
    c1 = (int)(line % n1);
    base = line * n2;
    stride = 1;
    len = n2;
  }
  auto off_axis = [&](long long v, int& j0, int& j1) -> long long {
    j0 = in0[v];
    j1 = D == 2 ? in1[v] : 0;
    const long long d0 = j0 - c0, d1 = D == 2 ? (long long)(j1 - c1) : 0ll;
    return d0 * d0 + d1 * d1;
  };
  // build
  int top = -1;
  long long g1 = 0, r1 = 0, g2 = 0, r2 = 0;      // the two top entries: (g2, r2) on top of (g1, r1)
  for (int p = 0; p < len; ++p) {
    const long long v = base + p * stride;
    if (in0[v] < 0) continue;
    int j0, j1;
    const long long wr = off_axis(v, j0, j1);
    while (top >= 1) {
      const long long a = g2 - g1, b = p - g2, c = a + b;
      if (c * r2 - b * r1 - a * wr - a * b * c <= 0) break;
      --top;
      g2 = g1; r2 = r1;
      if (top >= 1) { g1 = spos[base + (top - 1) * stride]; r1 = sr[base + (top - 1) * stride]; }
    }
    ++top;
    spos[base + top * stride] = (short)p;
    sr[base + top * stride] = (int)wr;
    g1 = g2; r1 = r2;
    g2 = p; r2 = wr;
  }
  // query
  int l = 0;
  long long gc = 0, rc = 0;
  if (top >= 0) { gc = spos[base]; rc = sr[base]; }
  for (int p = 0; p < len; ++p) {
    const long long v = base + p * stride;
    if (top < 0) {
      if (D == 1) { out0[v] = -1; out1[v] = -1; }
      else {
        if (o.sqdist) o.sqdist[v] = -1;
        if (o.dist) o.dist[v] = -1.0;
        if (o.indices) { o.indices[v] = -1; o.indices[v + (long long)n0 * n1 * n2] = -1; o.indices[v + 2ll * n0 * n1 * n2] = -1; }
        if (o.lin) o.lin[v] = -1;
        if (o.gather_out) o.gather_out[v] = 0;
      }
      continue;
    }
    long long d1 = (gc - p) * (gc - p) + rc;
    while (l < top) {
      const long long gn = spos[base + (l + 1) * stride], rn = sr[base + (l + 1) * stride];
      const long long d2 = (gn - p) * (gn - p) + rn;
      if (d1 <= d2) break;
      d1 = d2; gc = gn; rc = rn; ++l;
    }
    const long long site = base + gc * stride;
    const int j0 = in0[site];
    if (D == 1) {
      out0[v] = (short)j0;
      out1[v] = (short)gc;
    } else {
      const int j1 = in1[site];
      const long long n = (long long)n0 * n1 * n2;
      if (o.sqdist) o.sqdist[v] = (int)d1;
      if (o.dist) o.dist[v] = sqrt((double)d1);
      if (o.indices) { o.indices[v] = j0; o.indices[v + n] = j1; o.indices[v + 2 * n] = (int)gc; }
      if (o.lin) o.lin[v] = (int)(((long long)j0 * n1 + j1) * n2 + gc);
      if (o.gather_out) o.gather_out[v] = o.gather_mask[v] != 0 ? o.gather_src[((long long)j0 * n1 + j1) * n2 + gc] : 0;
    }
  }
}

size_t edt_workspace_bytes(int n0, int n1, int n2) { return measured(edt_ws, n0, n1, n2); }

// pass 0 with its status preset; shared with the passes in float64 of edt_sampling.hip, whose pass 0 is this one
int run_edt_pass0(const unsigned char* vol, bool invert, int n0, int n1, int n2, short* f0, int* status_dev, hipStream_t s) {
  if (status_dev) SEUNET_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(status_dev), 1, 1, s));
  const long long plane = (long long)n1 * n2;
  if (invert) edt_pass0_kernel<true><<<blocks_256(plane), 256, 0, s>>>(vol, n0, plane, f0, status_dev);
  else edt_pass0_kernel<false><<<blocks_256(plane), 256, 0, s>>>(vol, n0, plane, f0, status_dev);
  return 0;
}

int run_edt(const unsigned char* vol, bool invert, int n0, int n1, int n2, EdtOut o, int* status_dev, void* workspace, size_t ws_bytes,
            hipStream_t s) {
  SEUNET_CHECK(vol && workspace, "edt: null argument");
  if (volume_check("edt", n0, n1, n2, kEdtMaxExtent)) return 1;
  WsCarver carve(workspace);
  const EdtWs w = edt_ws(carve, n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "edt: workspace too small");
  if (run_edt_pass0(vol, invert, n0, n1, n2, w.f0, status_dev, s)) return 1;
  const long long l1 = (long long)n0 * n2, l2 = (long long)n0 * n1;
  edt_pass_kernel<1><<<blocks_256(l1), 256, 0, s>>>(w.f0, nullptr, n0, n1, n2, w.spos, w.sr, w.fa, w.fb, o);
  edt_pass_kernel<2><<<blocks_256(l2), 256, 0, s>>>(w.fa, w.fb, n0, n1, n2, w.spos, w.sr, nullptr, nullptr, o);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_edt(const unsigned char* vol, int n0, int n1, int n2, int* sqdist, double* dist, int* indices, int* status_dev,
               void* workspace, size_t ws_bytes, hipStream_t s) {
  return run_edt(vol, false, n0, n1, n2, EdtOut{sqdist, dist, indices, nullptr, nullptr, nullptr, nullptr}, status_dev, workspace, ws_bytes, s);
}

// ---- bit-packed candidate masks ---------------------------------------------------------------------------------------
// bit j of word w = voxel 64 w + j in raster order.  A wave covers one word.

__global__ void __launch_bounds__(256)
mask_bits_kernel(const unsigned char* __restrict__ m, long long n, u64* __restrict__ bits) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  const u64 b = __ballot(i < n && m[i < n ? i : 0] != 0);
  if ((threadIdx.x & 63) == 0 && i < n) bits[i >> 6] = b;
}

// loc_skeleton = skeleton != 0 and pred != 1 (where(skeleton * (1 - pred)));
// loc_small = skeleton == 0 or EDT(label)^2 < 4 (where(dis * skeleton < 2)).  A squared distance below 4 is one of 0..3,
// i.e. a zero label voxel inside the 3x3x3 neighbourhood (any farther zero voxel is at least 4 away): the exact predicate.
__global__ void __launch_bounds__(256)
hm_candidates_kernel(const unsigned char* __restrict__ label, const unsigned char* __restrict__ skel,
                     const unsigned char* __restrict__ pred, int n0, int n1, int n2, u64* __restrict__ skel_bits,
                     u64* __restrict__ small_bits) {
  const long long n = (long long)n0 * n1 * n2;
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  bool sk = false, sm = false;
  if (i < n) {
    const bool on = skel[i] != 0;
    sk = on && pred[i] != 1;
    sm = !on || label[i] == 0;
    if (!sm) {
      const Vox3 p = vox3(i, n1, n2);
      const int i0 = p.i0, i1 = p.i1, i2 = p.i2;
      for (int a = std::max(i0 - 1, 0); a <= std::min(i0 + 1, n0 - 1) && !sm; ++a)
        for (int b = std::max(i1 - 1, 0); b <= std::min(i1 + 1, n1 - 1) && !sm; ++b) {
          const unsigned char* row = label + ((long long)a * n1 + b) * n2;
          for (int c = std::max(i2 - 1, 0); c <= std::min(i2 + 1, n2 - 1); ++c) sm = sm || row[c] == 0;
        }
    }
  }
  const u64 bk = __ballot(sk), bm = __ballot(sm);
  if ((threadIdx.x & 63) == 0 && i < n) { skel_bits[i >> 6] = bk; small_bits[i >> 6] = bm; }
}

int launch_mask_bits(const unsigned char* mask, long long n, u64* bits, hipStream_t s) {
  SEUNET_CHECK(mask && bits && n >= 1, "mask_bits: bad argument");
  mask_bits_kernel<<<blocks_256(n), 256, 0, s>>>(mask, n, bits);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_hm_candidates(const unsigned char* label, const unsigned char* skel, const unsigned char* pred, int n0, int n1, int n2,
                         u64* skel_bits, u64* small_bits, hipStream_t s) {
  SEUNET_CHECK(label && skel && pred && skel_bits && small_bits, "hard_mining_candidates: null argument");
  if (volume_check("hard_mining_candidates", n0, n1, n2, kEdtMaxExtent)) return 1;
  const long long n = (long long)n0 * n1 * n2;
  hm_candidates_kernel<<<blocks_256(n), 256, 0, s>>>(label, skel, pred, n0, n1, n2, skel_bits, small_bits);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// ---- LIB weight (lib_weight.py:12-17, 36-53) ---------------------------------------------------------------------------
// 7x7x7 counts of non-zero label voxels, mode 'mirror' (d c b | a b c d | c b a), as three 7-tap passes on bytes; then
// table[count] * label in float32 (table[k] = -log10(float32(k) / 343), table[0] = -log10(1) = -0.0, built by the caller)
// and float16.  The counts are exact integers, as the reference's float32 sums of 0/1 values are.

struct LibTable { float v[344]; };

// The float32 value as computed, then rounded to float16 on its own: without the barrier the backend folds a product and the
// conversion into one mixed-precision fma (single rounding, and a +0 addend that turns -0 into +0), which numpy does not do.
__device__ __forceinline__ float f32_opaque(float x) {
  asm volatile("" : "+v"(x));
  return x;
}

__device__ __forceinline__ int mirror_index(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

// AX = 2: count of non-zero input voxels along axis 2; AX = 1: sum of the input counts along axis 1
template <int AX>
__global__ void __launch_bounds__(256)
box7_kernel(const unsigned char* __restrict__ in, int n0, int n1, int n2, unsigned char* __restrict__ out) {
  const long long n = (long long)n0 * n1 * n2;
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const int i2 = (int)(i % n2);     // (not vox3: the row index r itself is used)
  const long long r = i / n2;
  const int i1 = (int)(r % n1);
  int acc = 0;
  if (AX == 2) {
    const unsigned char* row = in + r * n2;
    for (int t = -3; t <= 3; ++t) acc += row[mirror_index(i2 + t, n2)] != 0;
  } else {
    const unsigned char* col = in + (i - (long long)i1 * n2);
    for (int t = -3; t <= 3; ++t) acc += col[(long long)mirror_index(i1 + t, n1) * n2];
  }
  out[i] = (unsigned char)acc;
}

__global__ void __launch_bounds__(256)
lib_weight_kernel(const unsigned char* __restrict__ cnt12, const unsigned char* __restrict__ label, int n0, int n1, int n2,
                  LibTable table, f16_t* __restrict__ out) {
  const long long plane = (long long)n1 * n2;
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= (long long)n0 * plane) return;
  const int i0 = (int)(i / plane);
  const long long rem = i - i0 * plane;
  int c = 0;
  for (int t = -3; t <= 3; ++t) c += cnt12[mirror_index(i0 + t, n0) * plane + rem];
  out[i] = (f16_t)f32_opaque(table.v[c] * (label[i] != 0 ? 1.0f : 0.0f));
}

size_t lib_weight_workspace_bytes(int n0, int n1, int n2) { return measured(lib_weight_ws, n0, n1, n2); }

int launch_lib_weight(const unsigned char* label, int n0, int n1, int n2, const float* table, void* out, void* workspace,
                      size_t ws_bytes, hipStream_t s) {
  SEUNET_CHECK(label && table && out && workspace, "lib_weight: null argument");
  if (volume_check("lib_weight", n0, n1, n2, kEdtMaxExtent)) return 1;
  WsCarver carve(workspace);
  const LibWeightWs w = lib_weight_ws(carve, n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "lib_weight: workspace too small");
  LibTable t;
  for (int k = 0; k < 344; ++k) t.v[k] = table[k];
  const unsigned blocks = blocks_256((long long)n0 * n1 * n2);
  box7_kernel<2><<<blocks, 256, 0, s>>>(label, n0, n1, n2, w.c2);
  box7_kernel<1><<<blocks, 256, 0, s>>>(w.c2, n0, n1, n2, w.c12);
  lib_weight_kernel<<<blocks, 256, 0, s>>>(w.c12, label, n0, n1, n2, t, reinterpret_cast<f16_t*>(out));
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// ---- break weight (weight_br.py:113-177, save_weight_break with the skeleton given) ------------------------------------
// Volumes are 0/1 bytes (non-zero = 1).  Steps, in the reference's order:
//   fn_skel = label & !pred & skeleton;  (edt, inds) = EDT(1 - skeleton) with indices;  hm = fn_skel[inds] * label;
//   loc = hm > 0;  f = loc * edt * (1 - skeleton);  maxf = max f  (0: all zeros, empty br_skel);
//   D = (-((1 / maxf) * f) + 1) * loc;  w_hm = f16(hm^2 * D^2)  (float64, no contraction, direct float64 -> float16);
//   br_skel = union of the 26-connected components of fn_skel with no voxel whose 3x3x3 skeleton count (mode 'reflect') is 2;
//   br_label = br_skel[inds] * label;  shell = dilate6(br_label) - br_label;  e = EDT(1 - shell);
//   w_br = f16(min(br_label * e, 2));  out = f16(f16(f16(f16(f16(w_br + w_hm) * f16(0.7)) + 1) - f16(0.7)) * hm),
//   every float16 operation done in float32 and rounded, as numpy's half loops do.
// br_label * e only matters below 2: e^2 in {1, 2, 3}, i.e. a shell voxel inside the 3x3x3 neighbourhood (anything farther is
// at least 2 away and clips to 2), so the second EDT is that neighbourhood test.

__device__ __forceinline__ unsigned short f64_to_f16_bits(double x) {     // round to nearest even, directly
  const u64 b = __builtin_bit_cast(u64, x);
  const unsigned short sign = (unsigned short)((b >> 48) & 0x8000u);
  const int ex = (int)((b >> 52) & 0x7ff);
  const u64 man = b & ((1ull << 52) - 1);
  if (ex == 0x7ff) return sign | (man ? 0x7e00u : 0x7c00u);
  if (ex == 0) return sign;                                   // double subnormals are far below half's range
  const int e = ex - 1023;
  const u64 sig = (1ull << 52) | man;
  int shift = 42;                                             // 52 - 10 mantissa bits
  if (e < -14) shift += -14 - e;                              // half subnormal
  if (shift > 53) return sign;                                // below half of the smallest subnormal
  u64 h = sig >> shift;
  const u64 rem = sig & ((1ull << shift) - 1), half = 1ull << (shift - 1);
  if (rem > half || (rem == half && (h & 1))) ++h;
  if (e < -14) return sign | (unsigned short)h;               // h == 1024 is the smallest normal: same bits
  int eh = e + 15;
  if (h == 2048) { h = 1024; ++eh; }
  if (eh >= 31) return sign | 0x7c00u;
  return sign | (unsigned short)(eh << 10) | (unsigned short)(h & 0x3ff);
}

__device__ __forceinline__ float h16(float x) { return (float)(f16_t)f32_opaque(x); }   // one numpy float16 operation's rounding

__global__ void __launch_bounds__(256)
fnskel_kernel(const unsigned char* __restrict__ label, const unsigned char* __restrict__ pred, const unsigned char* __restrict__ skel,
              long long n, unsigned char* __restrict__ fn) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  fn[i] = (label[i] != 0 && pred[i] == 0 && skel[i] != 0) ? 1 : 0;
}

__device__ __forceinline__ long long sq_to(long long i, int f, int n1, int n2) {   // squared distance voxel i -> voxel f
  const long long d2 = i % n2 - f % n2;
  const long long d1 = (i / n2) % n1 - (f / n2) % n1;
  const long long d0 = i / ((long long)n1 * n2) - f / ((long long)n1 * n2);
  return d0 * d0 + d1 * d1 + d2 * d2;
}

__global__ void __launch_bounds__(256)
br_maxf_kernel(const int* __restrict__ lin, const unsigned char* __restrict__ fn, const unsigned char* __restrict__ label,
               const unsigned char* __restrict__ skel, int n0, int n1, int n2, u64* __restrict__ maxf) {
  const long long n = (long long)n0 * n1 * n2;
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  double f = 0.0;
  if (i < n) {
    const int ft = lin[i];
    if (ft >= 0 && fn[ft] && label[i]) f = sqrt((double)sq_to(i, ft, n1, n2)) * (1.0 - (skel[i] != 0 ? 1.0 : 0.0));
  }
  const u64 key = wave_max(__builtin_bit_cast(u64, f));        // non-negative doubles order like their bit patterns
  if ((threadIdx.x & 63) == 0 && key) atomicMax(maxf, key);
}

// a component of fn_skel that has a skeleton end point (3x3x3 count, centre included, == 2) is not a break
__global__ void __launch_bounds__(256)
br_endpoint_kernel(const int* __restrict__ L, const unsigned char* __restrict__ skel, int n0, int n1, int n2,
                   unsigned char* __restrict__ flag) {
  const long long n = (long long)n0 * n1 * n2;
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n || L[i] < 0) return;
  if (count27_clamped(skel, vox3(i, n1, n2), n0, n1, n2) == 2) flag[L[i]] = 1;   // 'reflect' at radius 1 repeats the edge voxel
}

__global__ void __launch_bounds__(256)
br_skel_kernel(const int* __restrict__ L, const unsigned char* __restrict__ flag, long long n, unsigned char* __restrict__ brs) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  brs[i] = (L[i] >= 0 && !flag[L[i]]) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
br_label_kernel(const int* __restrict__ lin, const unsigned char* __restrict__ brs, const unsigned char* __restrict__ label, long long n,
                unsigned char* __restrict__ brl) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const int ft = lin[i];
  brl[i] = (ft >= 0 && brs[ft] && label[i]) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
br_shell_kernel(const unsigned char* __restrict__ brl, int n0, int n1, int n2, unsigned char* __restrict__ shell) {
  const long long n = (long long)n0 * n1 * n2;
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const Vox3 v = vox3(i, n1, n2);
  const int i0 = v.i0, i1 = v.i1, i2 = v.i2;
  const long long p = (long long)n1 * n2;
  const bool on = !brl[i] && ((i2 > 0 && brl[i - 1]) || (i2 + 1 < n2 && brl[i + 1]) || (i1 > 0 && brl[i - n2]) ||
                              (i1 + 1 < n1 && brl[i + n2]) || (i0 > 0 && brl[i - p]) || (i0 + 1 < n0 && brl[i + p]));
  shell[i] = on ? 1 : 0;
}

__global__ void __launch_bounds__(256)
br_final_kernel(const int* __restrict__ lin, const unsigned char* __restrict__ fn, const unsigned char* __restrict__ label,
                const unsigned char* __restrict__ skel, const unsigned char* __restrict__ brs, const unsigned char* __restrict__ brl,
                const unsigned char* __restrict__ shell, const u64* __restrict__ maxf_bits, int n0, int n1, int n2,
                unsigned short* __restrict__ w_out, unsigned char* __restrict__ brs_out) {
  const long long n = (long long)n0 * n1 * n2;
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const double maxf = __builtin_bit_cast(double, *maxf_bits);
  if (maxf == 0.0) { w_out[i] = 0; brs_out[i] = 0; return; }  // weight_br.py:141-148 (an empty loc_break here)
  brs_out[i] = brs[i];
  const int ft = lin[i];
  const bool hm = ft >= 0 && fn[ft] && label[i];
  if (!hm) { w_out[i] = 0; return; }                           // (... * hard_mining = +0)
  // w_hm
  const double edt = sqrt((double)sq_to(i, ft, n1, n2));
  const double f = edt * (1.0 - (skel[i] != 0 ? 1.0 : 0.0));
  const double d = (-((1.0 / maxf) * f) + 1.0) * 1.0;
  const float w_hm = (float)__builtin_bit_cast(f16_t, f64_to_f16_bits(1.0 * (d * d)));
  // w_br
  float w_br = 0.0f;
  if (brl[i]) {
    const Vox3 v = vox3(i, n1, n2);
    const int i0 = v.i0, i1 = v.i1, i2 = v.i2;
    int best = 4;
    for (int a = -1; a <= 1; ++a)
      for (int b = -1; b <= 1; ++b)
        for (int c = -1; c <= 1; ++c) {
          const int x0 = i0 + a, x1 = i1 + b, x2 = i2 + c;
          if (x0 < 0 || x0 >= n0 || x1 < 0 || x1 >= n1 || x2 < 0 || x2 >= n2) continue;
          if (shell[((long long)x0 * n1 + x1) * n2 + x2]) best = std::min(best, a * a + b * b + c * c);
        }
    const double e = best >= 4 ? 2.0 : sqrt((double)best);
    w_br = (float)__builtin_bit_cast(f16_t, f64_to_f16_bits(e));
  }
  const float lam = h16(0.7f);
  float t = h16(w_br + w_hm);
  t = h16(t * lam);
  t = h16(t + 1.0f);
  t = h16(t - lam);
  t = h16(t * 1.0f);
  w_out[i] = __builtin_bit_cast(unsigned short, (f16_t)t);
}

size_t break_weight_workspace_bytes(int n0, int n1, int n2) { return measured(break_weight_ws, n0, n1, n2); }

int launch_break_weight(const unsigned char* label, const unsigned char* pred, const unsigned char* skel, int n0, int n1, int n2,
                        void* w_br, unsigned char* br_skel, int* status_dev, void* workspace, size_t ws_bytes, hipStream_t s) {
  SEUNET_CHECK(label && pred && skel && w_br && br_skel && workspace, "break_weight: null argument");
  if (volume_check("break_weight", n0, n1, n2, kEdtMaxExtent)) return 1;
  WsCarver carve(workspace);
  const BreakWeightWs w = break_weight_ws(carve, n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "break_weight: workspace too small");
  const long long n = (long long)n0 * n1 * n2;
  const unsigned blocks = blocks_256(n);
  SEUNET_HIP(hipMemsetAsync(w.flag, 0, (size_t)n, s));
  SEUNET_HIP(hipMemsetAsync(w.maxf, 0, sizeof(u64), s));
  fnskel_kernel<<<blocks, 256, 0, s>>>(label, pred, skel, n, w.fn);
  if (run_edt(skel, true, n0, n1, n2, EdtOut{nullptr, nullptr, nullptr, w.lin, nullptr, nullptr, nullptr}, status_dev, w.edt.f0, w.edt_bytes, s))
    return 1;
  br_maxf_kernel<<<blocks, 256, 0, s>>>(w.lin, w.fn, label, skel, n0, n1, n2, w.maxf);
  cc_label26(w.fn, n0, n1, n2, w.labels, s);
  br_endpoint_kernel<<<blocks, 256, 0, s>>>(w.labels, skel, n0, n1, n2, w.flag);
  br_skel_kernel<<<blocks, 256, 0, s>>>(w.labels, w.flag, n, w.brs);
  br_label_kernel<<<blocks, 256, 0, s>>>(w.lin, w.brs, label, n, w.brl);
  br_shell_kernel<<<blocks, 256, 0, s>>>(w.brl, n0, n1, n2, w.shell);
  br_final_kernel<<<blocks, 256, 0, s>>>(w.lin, w.fn, label, skel, w.brs, w.brl, w.shell, w.maxf, n0, n1, n2,
                                         reinterpret_cast<unsigned short*>(w_br), br_skel);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
