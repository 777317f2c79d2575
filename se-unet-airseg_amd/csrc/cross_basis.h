// The in-plane basis of a section perpendicular to a unit tangent, shared by the section pass (cross_section.hip) and the wall
// pass (airway_wall.hip) so that both stand in the same frame bit for bit (include/seunet_hip.h: `basis`).
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>

// the oracle's float64 arithmetic operation by operation
#pragma clang fp contract(off)

namespace seunet {

// u = normalise(e_a - t_a t) with a the index of smallest |t_a| (the lowest on a tie), v = t x u
__device__ __forceinline__ void cross_basis(const double (&t)[3], double (&u)[3], double (&v)[3]) {
  int a = 0;
  double least = fabs(t[0]);
  if (fabs(t[1]) < least) { a = 1; least = fabs(t[1]); }
  if (fabs(t[2]) < least) a = 2;
  const double ta = a == 0 ? t[0] : a == 1 ? t[1] : t[2];
  double w[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) w[q] = (q == a ? 1.0 : 0.0) - ta * t[q];
  const double len = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
  for (int q = 0; q < 3; ++q) u[q] = w[q] / len;
  v[0] = t[1] * u[2] - t[2] * u[1];
  v[1] = t[2] * u[0] - t[0] * u[2];
  v[2] = t[0] * u[1] - t[1] * u[0];
}

}  // namespace seunet
