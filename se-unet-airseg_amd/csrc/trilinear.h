// Trilinear index helpers with PyTorch's align_corners=True semantics, shared by the x2 up-sampling of feature maps
// (resample.hip) and the interpolation of the deep-supervision heads (heads.hip).
#pragma once
#include "seunet_common.h"

namespace seunet {

__device__ __forceinline__ float ac_scale(int in, int out) {
  return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
}
__device__ __forceinline__ void ac_src(int o, float rs, int in, int& i0, int& i1, float& lam) {
  const float src = rs * (float)o;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  lam = src - (float)i0;
}
// output indices that can touch input index i
__device__ __forceinline__ void ac_range(int i, float rs, int out, int& lo, int& hi) {
  if (rs <= 0.f) { lo = 0; hi = out - 1; return; }
  lo = (int)floorf((float)(i - 1) / rs) - 1;
  hi = (int)ceilf((float)(i + 1) / rs) + 1;
  if (lo < 0) lo = 0;
  if (hi > out - 1) hi = out - 1;
}
__device__ __forceinline__ float ac_weight(int o, int i, float rs, int in) {
  int i0, i1; float lam;
  ac_src(o, rs, in, i0, i1, lam);
  return (i0 == i ? 1.f - lam : 0.f) + (i1 == i ? lam : 0.f);
}

}  // namespace seunet
