// The exact Euclidean distance transform with voxel spacing: scipy.ndimage.distance_transform_edt(volume, sampling=s,
// return_indices=True) on the device.
//
// scipy runs its feature transform (ni_morphology.c) in float64 and computes the distances from the indices in numpy.  The order
// of operations below is the contract of DESIGN.md section 3k, restated in plain Python by tests/edt_sampling_oracle.py and
// recorded from scipy itself in tests/golden/edt_sampling_known.npz; every product and sum is rounded on its own.
//   pass 0   along axis 0 the off-axis terms are zero: the pop test never pops and the query orders sites by |t|, since
//            (t s0)^2 is strictly monotone in |t| up to 32767 and ties are exactly equal.  This is the integer pass 0 of
//            edt.hip, run as it is (run_edt_pass0).
//   pass 1/2 one lane per line, as edt_pass_kernel.  The stack of a line lives in a volume-shaped workspace at the line's own
//            voxels and holds POSITIONS only (2 bytes per voxel).  The off-line term of a site (wR / uR / vR of the contract)
//            is recomputed from the site's int16 features where it is needed: it is the same double whenever it is formed, the
//            top two entries' terms stay in registers, and a recomputation reads 2 or 4 bytes from a line of memory the build
//            scan has just read, where a stored double would add 8 bytes per voxel of workspace and its traffic.
//   query    delta = (t0^2 + t1^2) + t2^2 in ascending axis order, which is the site's off-line term plus the squared on-line
//            term in both passes (pass 1: t2 = 0 and x + 0.0 = x); the last pass's delta of the chosen site is numpy's squared
//            distance, so dist = sqrt(delta).
// Between passes the features are int16 (extents <= 32767), as in edt.hip.
#include "volume.h"

// neither scipy's C (as built for x86-64) nor numpy contracts a * b + c into a fused multiply-add; hipcc does by default
#pragma clang fp contract(off)

namespace seunet {

// pass D (1 or 2) along axis D.  in0 / in1: features along axes 0 / 1 of the previous passes (in1 for D == 2 only).
// D == 1 writes out0 / out1 (features along axes 0 / 1); D == 2 writes the final outputs.  sd: the spacing along axis D.
template <int D>
__global__ void __launch_bounds__(256)
edt_sampling_pass_kernel(const short* __restrict__ in0, const short* __restrict__ in1, int n0, int n1, int n2, double s0, double s1,
                         double sd, short* __restrict__ spos, short* __restrict__ out0, short* __restrict__ out1, EdtSamplingOut o) {
  const long long line = blockIdx.x * 256ll + threadIdx.x;
  long long base, stride;
  int len, c0, c1;
  if (D == 1) {            // line (i0, i2)
    if (line >= (long long)n0 * n2) return;
    c0 = (int)(line / n2);
    c1 = 0;
    base = (long long)c0 * n1 * n2 + line % n2;
    stride = n2;
    len = n1;
  } else {                 // line (i0, i1)
    if (line >= (long long)n0 * n1) return;
    c0 = (int)(line / n1);
    c1 = (int)(line % n1);
    base = line * n2;
    stride = 1;
    len = n2;
  }
  // the off-line term of the site at voxel v: sum over the axes other than D, ascending, of ((feature - coordinate) * spacing)^2
  auto off_axis = [&](long long v) -> double {
    const double t0 = (double)(in0[v] - c0) * s0;
    if (D == 1) return t0 * t0;
    const double t1 = (double)(in1[v] - c1) * s1;
    return t0 * t0 + t1 * t1;
  };
  // build
  int top = -1;
  int g1 = 0, g2 = 0;                              // the two top entries: g2 on top of g1
  double r1 = 0.0, r2 = 0.0;                       // their off-line terms (uR, vR)
  for (int p = 0; p < len; ++p) {
    const long long v = base + p * stride;
    if (in0[v] < 0) continue;
    const double wr = off_axis(v);
    while (top >= 1) {
      const double a = (double)(g2 - g1) * sd, b = (double)(p - g2) * sd, c = a + b;
      if (c * r2 - b * r1 - a * wr - a * b * c <= 0.0) break;
      --top;
      g2 = g1; r2 = r1;
      if (top >= 1) { g1 = spos[base + (top - 1) * stride]; r1 = off_axis(base + g1 * stride); }
    }
    ++top;
    spos[base + top * stride] = (short)p;
    g1 = g2; r1 = r2;
    g2 = p; r2 = wr;
  }
  // query
  const long long n = (long long)n0 * n1 * n2;
  int l = 0, gc = 0;
  double rc = 0.0;
  if (top >= 0) { gc = spos[base]; rc = off_axis(base + gc * stride); }
  for (int p = 0; p < len; ++p) {
    const long long v = base + p * stride;
    if (top < 0) {
      if (D == 1) { out0[v] = -1; out1[v] = -1; }
      else {
        if (o.dist) o.dist[v] = -1.0;
        if (o.indices) { o.indices[v] = -1; o.indices[v + n] = -1; o.indices[v + 2 * n] = -1; }
        if (o.lin) o.lin[v] = -1;
      }
      continue;
    }
    const double tc = (double)(gc - p) * sd;
    double d1 = rc + tc * tc;
    while (l < top) {
      const int gn = spos[base + (l + 1) * stride];
      const double rn = off_axis(base + gn * stride), tn = (double)(gn - p) * sd;
      const double d2 = rn + tn * tn;
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
      if (o.dist) o.dist[v] = sqrt(d1);
      if (o.indices) { o.indices[v] = j0; o.indices[v + n] = j1; o.indices[v + 2 * n] = gc; }
      if (o.lin) o.lin[v] = (int)(((long long)j0 * n1 + j1) * n2 + gc);
    }
  }
}

size_t edt_sampling_workspace_bytes(int n0, int n1, int n2) { return measured(edt_sampling_ws, n0, n1, n2); }

int launch_edt_sampling(const unsigned char* vol, int n0, int n1, int n2, double s0, double s1, double s2, EdtSamplingOut o,
                        int* status_dev, void* workspace, size_t ws_bytes, hipStream_t s) {
  SEUNET_CHECK(vol && workspace, "edt_sampling: null argument");
  if (volume_check("edt_sampling", n0, n1, n2, kEdtMaxExtent)) return 1;
  SEUNET_CHECK(s0 > 0.0 && s1 > 0.0 && s2 > 0.0 && s0 < HUGE_VAL && s1 < HUGE_VAL && s2 < HUGE_VAL,
               "edt_sampling: the sampling must be three positive finite numbers, got (%g, %g, %g)", s0, s1, s2);
  WsCarver carve(workspace);
  const EdtSamplingWs w = edt_sampling_ws(carve, n0, n1, n2);
  SEUNET_CHECK(ws_bytes >= carve.bytes(), "edt_sampling: workspace too small");
  if (run_edt_pass0(vol, false, n0, n1, n2, w.f0, status_dev, s)) return 1;
  const long long l1 = (long long)n0 * n2, l2 = (long long)n0 * n1;
  edt_sampling_pass_kernel<1><<<blocks_256(l1), 256, 0, s>>>(w.f0, nullptr, n0, n1, n2, s0, s1, s1, w.spos, w.fa, w.fb, o);
  edt_sampling_pass_kernel<2><<<blocks_256(l2), 256, 0, s>>>(w.fa, w.fb, n0, n1, n2, s0, s1, s2, w.spos, nullptr, nullptr, o);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
