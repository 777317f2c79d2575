// x2 trilinear (align_corners=True) up-sampling of feature maps and its transpose (gfx950).  HBM-bound; one lane moves
// 8 channels (16/32 B).
//
//   up-sampling   reference SE_UNet.py:136-138 (nn.Upsample x2 trilinear align_corners=True)
#include "seunet_common.h"
#include "trilinear.h"

namespace seunet {

// ---------------- x2 trilinear up-sampling of feature maps ------------------------------------
template <typename T>
__global__ void upsample2_fwd_kernel(const T* __restrict__ in, int C, T* __restrict__ out, int D, int H,
                                     int W, long long total) {
  const int G = C / 8, Do = 2 * D, Ho = 2 * H, Wo = 2 * W;
  const float rz = ac_scale(D, Do), ry = ac_scale(H, Ho), rx = ac_scale(W, Wo);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int g = (int)(i % G);
    long long r = i / G;
    const int xo = (int)(r % Wo); r /= Wo;
    const int yo = (int)(r % Ho); r /= Ho;
    const int zo = (int)(r % Do);
    const long long n = r / Do;
    int z0, z1, y0, y1, x0, x1; float lz, ly, lx;
    ac_src(zo, rz, D, z0, z1, lz);
    ac_src(yo, ry, H, y0, y1, ly);
    ac_src(xo, rx, W, x0, x1, lx);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int z = (k & 4) ? z1 : z0, y = (k & 2) ? y1 : y0, x = (k & 1) ? x1 : x0;
      const float w = ((k & 4) ? lz : 1.f - lz) * ((k & 2) ? ly : 1.f - ly) * ((k & 1) ? lx : 1.f - lx);
      float v[8];
      load8(in + ((((n * D + z) * H + y) * W + x) * (long long)C) + g * 8, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += w * v[j];
    }
    store8(out + ((((n * Do + zo) * Ho + yo) * Wo + xo) * (long long)C) + g * 8, acc);
  }
}

// Tiled separable form (the one the network uses).  The kernel above issues 8 16-byte loads per stored 16 bytes and is bound
// by the texture path (0.36 ms for the 32-channel 64^3 -> 128^3 map, 1.7 TB/s).  Here a block produces the 2 x 2 output
// rows (zo, yo) in {2zb, 2zb+1} x {2yb, 2yb+1} over 128 fine x: phase A blends the <= 3 x 3 coarse (z, y) rows those four
// output rows draw on -- each coarse 16-byte piece is loaded ONCE per block -- into four z/y-interpolated coarse rows in LDS
// (f32); phase B interpolates along x from LDS and stores coalesced: ~1.2 loads per store instead of 8.
constexpr int UF_XF = 128, UF_XC = 68;   // fine x per block; coarse x a block can touch (128 * 63/127 + 2 < 68)
template <typename T>
__global__ void __launch_bounds__(256)
upsample2_fwd_tiled_kernel(const T* __restrict__ in, int C, T* __restrict__ out, int D, int H, int W) {
  extern __shared__ __attribute__((aligned(16))) float uf[];   // [4 rows][UF_XC][C]
  const int G = C / 8, Do = 2 * D, Ho = 2 * H, Wo = 2 * W;
  const float rz = ac_scale(D, Do), ry = ac_scale(H, Ho), rx = ac_scale(W, Wo);
  const int xf0 = blockIdx.x * UF_XF;
  const int nxf = (Wo - xf0 < UF_XF) ? Wo - xf0 : UF_XF;
  const int yb = blockIdx.y, zb = blockIdx.z % D;
  const long long n = blockIdx.z / D;
  // coarse rows and weights of the two zo / yo of this block
  int zs[2][2], ys[2][2]; float lzs[2], lys[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    ac_src(2 * zb + k, rz, D, zs[k][0], zs[k][1], lzs[k]);
    ac_src(2 * yb + k, ry, H, ys[k][0], ys[k][1], lys[k]);
  }
  const int zc0 = zs[0][0], nzc = zs[1][1] - zc0 + 1;         // distinct coarse z: zc0 .. zc0 + nzc - 1 (<= 3)
  const int yc0 = ys[0][0], nyc = ys[1][1] - yc0 + 1;
  int xc0, xc1, t0, t1; float tl;
  ac_src(xf0, rx, W, xc0, t0, tl);
  ac_src(xf0 + nxf - 1, rx, W, t1, xc1, tl);
  const int nxc = xc1 - xc0 + 1;                               // <= UF_XC
  // phase A
  for (int item = threadIdx.x; item < nxc * G; item += 256) {
    const int g = item % G, xi = item / G;
    float acc[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[r][j] = 0.f;
    for (int zi = 0; zi < nzc; ++zi) {
      const int z = zc0 + zi;
      float wz[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) wz[k] = (zs[k][0] == z ? 1.f - lzs[k] : 0.f) + (zs[k][1] == z ? lzs[k] : 0.f);
      for (int yi = 0; yi < nyc; ++yi) {
        const int y = yc0 + yi;
        float v[8];
        load8(in + ((((n * D + z) * H + y) * W + (xc0 + xi)) * (long long)C) + g * 8, v);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const float wy = (ys[k][0] == y ? 1.f - lys[k] : 0.f) + (ys[k][1] == y ? lys[k] : 0.f);
#pragma unroll
          for (int kz = 0; kz < 2; ++kz) {
            const float w = wz[kz] * wy;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[kz * 2 + k][j] += w * v[j];
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float* q = uf + ((r * UF_XC + xi) * C) + g * 8;
      store8(q, acc[r]);
    }
  }
  __syncthreads();
  // phase B
  for (int item = threadIdx.x; item < 4 * nxf * G; item += 256) {
    const int g = item % G;
    int r2 = item / G;
    const int xo = xf0 + r2 % nxf, r = r2 / nxf;                // r = kz * 2 + ky
    int x0, x1; float lx;
    ac_src(xo, rx, W, x0, x1, lx);
    const float* q0 = uf + ((r * UF_XC + (x0 - xc0)) * C) + g * 8;
    const float* q1 = uf + ((r * UF_XC + (x1 - xc0)) * C) + g * 8;
    const float4 a0 = reinterpret_cast<const float4*>(q0)[0], b0 = reinterpret_cast<const float4*>(q0)[1];
    const float4 a1 = reinterpret_cast<const float4*>(q1)[0], b1 = reinterpret_cast<const float4*>(q1)[1];
    const float w0 = 1.f - lx;
    float o[8] = {w0 * a0.x + lx * a1.x, w0 * a0.y + lx * a1.y, w0 * a0.z + lx * a1.z, w0 * a0.w + lx * a1.w,
                  w0 * b0.x + lx * b1.x, w0 * b0.y + lx * b1.y, w0 * b0.z + lx * b1.z, w0 * b0.w + lx * b1.w};
    const int zo = 2 * zb + (r >> 1), yo = 2 * yb + (r & 1);
    store8(out + ((((n * Do + zo) * Ho + yo) * Wo + xo) * (long long)C) + g * 8, o);
  }
}

// z-marching form of the forward (the one the network uses for C = 32 / 64 / 128).  A block owns two fine rows x XF fine
// columns (XF * C = 4096) and a run of ZSF fine planes.  Each thread keeps its four (row, column, 8 channels) items'
// values at two consecutive COARSE planes in registers: walking the coarse planes once, it blends the new plane's four
// y/x corners from a small LDS image of the coarse rows (double-buffered, one barrier per coarse plane) and emits the
// fine planes between the two coarse planes as (1 - lz) * previous + lz * current.  Coarse rows are fetched ~2.3 times
// in all instead of ~9, the y/x blend is done once per coarse plane instead of once per fine plane, and every thread has
// the same amount of work.
constexpr int UFM_XC = 68, UFM_ZSF = 16;
template <typename T>
__global__ void __launch_bounds__(256)
upsample2_fwd_march_kernel(const T* __restrict__ in, int C, T* __restrict__ out, int D, int H, int W, int XF) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ufm_raw[];
  T* tile = reinterpret_cast<T*>(ufm_raw);                     // [2 buffers][3 coarse rows][UFM_XC][C]
  const int G = C / 8, Do = 2 * D, Ho = 2 * H, Wo = 2 * W;
  const float rz = ac_scale(D, Do), ry = ac_scale(H, Ho), rx = ac_scale(W, Wo);
  const TileIdx3 tl = xcd_contiguous_tile3();                  // (round 4: neighbouring tiles on one XCD, the halo in one L2)
  const int xf0 = tl.x * XF;
  const int nxf = (Wo - xf0 < XF) ? Wo - xf0 : XF;
  const int yb = tl.y;
  const int nseg = (Do + UFM_ZSF - 1) / UFM_ZSF;
  const int seg = tl.z % nseg;
  const long long n = tl.z / nseg;
  const int zf_a = seg * UFM_ZSF, zf_b = zf_a + UFM_ZSF < Do ? zf_a + UFM_ZSF : Do;
  int i0, i1; float lam;
  // coarse rows / columns under the block
  int ya0, ya1, yb0, yb1; float lya, lyb;
  ac_src(2 * yb, ry, H, ya0, ya1, lya);
  ac_src(2 * yb + 1, ry, H, yb0, yb1, lyb);
  const int yc0 = ya0, nyc = yb1 - yc0 + 1;                    // <= 3
  int xc0, xc1, t0;
  ac_src(xf0, rx, W, xc0, t0, lam);
  ac_src(xf0 + nxf - 1, rx, W, t0, xc1, lam);
  const int nxc = xc1 - xc0 + 1;                               // <= UFM_XC
  const int buf_elems = 3 * UFM_XC * C;
  // this thread's four items: fine row, fine column, channel group -> four corner offsets in a tile buffer and weights
  constexpr int NI = 4;
  int o00[NI], o01[NI], o10[NI], o11[NI];
  float w00[NI], w01[NI], w10[NI], w11[NI];
  long long oofs[NI];
  bool live[NI];
#pragma unroll
  for (int it = 0; it < NI; ++it) {
    const int item = threadIdx.x + 256 * it;
    const int g = item % G;
    const int r = item / G;
    const int fx = r % XF, fy = r / XF;                        // fy in {0, 1}
    live[it] = fx < nxf && fy < 2;
    const int xo = xf0 + (fx < nxf ? fx : 0);
    int x0, x1; float lx;
    ac_src(xo, rx, W, x0, x1, lx);
    const int y0 = fy ? yb0 : ya0, y1 = fy ? yb1 : ya1;
    const float ly = fy ? lyb : lya;
    o00[it] = ((y0 - yc0) * UFM_XC + (x0 - xc0)) * C + g * 8;
    o01[it] = ((y0 - yc0) * UFM_XC + (x1 - xc0)) * C + g * 8;
    o10[it] = ((y1 - yc0) * UFM_XC + (x0 - xc0)) * C + g * 8;
    o11[it] = ((y1 - yc0) * UFM_XC + (x1 - xc0)) * C + g * 8;
    w00[it] = (1.f - ly) * (1.f - lx); w01[it] = (1.f - ly) * lx; w10[it] = ly * (1.f - lx); w11[it] = ly * lx;
    oofs[it] = (((n * Do) * Ho + (2 * yb + (fy & 1))) * (long long)Wo + xo) * C + g * 8;   // + zo * Ho * Wo * C
  }
  const long long oplane = (long long)Ho * Wo * C;
  // coarse planes the segment needs
  ac_src(zf_a, rz, D, i0, i1, lam);
  const int zc_first = i0;
  ac_src(zf_b - 1, rz, D, i0, i1, lam);
  const int zc_last = i1;
  auto stage = [&](int zc, int buf) {          // coarse rows yc0.. of plane zc -> tile[buf]
    T* tb = tile + buf * buf_elems;
    for (int item = threadIdx.x; item < nyc * nxc * G; item += 256) {
      const int g = item % G;
      const int r = item / G;
      const int xi = r % nxc, yi = r / nxc;
      Pack8<T> v;
      load8p(in + ((((n * D + zc) * H + (yc0 + yi)) * (long long)W + (xc0 + xi)) * C) + g * 8, v);
      *reinterpret_cast<Pack8<T>*>(tb + (yi * UFM_XC + xi) * C + g * 8) = v;
    }
  };
  float pprev[NI][8], pcur[NI][8];
#pragma unroll
  for (int it = 0; it < NI; ++it)
#pragma unroll
    for (int j = 0; j < 8; ++j) pprev[it][j] = pcur[it][j] = 0.f;
  int zo = zf_a;
  stage(zc_first, 0);
  __syncthreads();
  int buf = 0;
  for (int zc = zc_first; zc <= zc_last; ++zc) {
    if (zc < zc_last) stage(zc + 1, buf ^ 1);                 // next coarse plane into the other buffer (read after the barrier)
    const T* tb = tile + buf * buf_elems;
#pragma unroll
    for (int it = 0; it < NI; ++it) {
      float a[8], b[8], c[8], d[8];
      Pack8<T> k;
      k = *reinterpret_cast<const Pack8<T>*>(tb + o00[it]); unpack8(k, a);
      k = *reinterpret_cast<const Pack8<T>*>(tb + o01[it]); unpack8(k, b);
      k = *reinterpret_cast<const Pack8<T>*>(tb + o10[it]); unpack8(k, c);
      k = *reinterpret_cast<const Pack8<T>*>(tb + o11[it]); unpack8(k, d);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        pprev[it][j] = pcur[it][j];
        pcur[it][j] = w00[it] * a[j] + w01[it] * b[j] + w10[it] * c[j] + w11[it] * d[j];
      }
    }
    // fine planes between coarse planes zc - 1 and zc (or clamped onto zc)
    while (zo < zf_b) {
      ac_src(zo, rz, D, i0, i1, lam);
      const bool between = i1 == zc && i0 == zc - 1, on = i0 == zc && i1 == zc;
      if (!between && !on) break;
      const float wp = between ? 1.f - lam : 0.f, wc = between ? lam : 1.f;
#pragma unroll
      for (int it = 0; it < NI; ++it) {
        if (!live[it]) continue;
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = wp * pprev[it][j] + wc * pcur[it][j];
        store8(out + oofs[it] + zo * oplane, o);
      }
      ++zo;
    }
    __syncthreads();                                          // the staged plane is complete; this plane's buffer is free
    buf ^= 1;
  }
}

// gather form of the transposed interpolation: one lane per (input voxel, 8 channels)
template <typename T>
__global__ void upsample2_bwd_kernel(const T* __restrict__ g_out, int C, T* g_in, int accumulate, int D,
                                     int H, int W, long long total) {
  const int G = C / 8, Do = 2 * D, Ho = 2 * H, Wo = 2 * W;
  const float rz = ac_scale(D, Do), ry = ac_scale(H, Ho), rx = ac_scale(W, Wo);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int g = (int)(i % G);
    long long r = i / G;
    const int x = (int)(r % W); r /= W;
    const int y = (int)(r % H); r /= H;
    const int z = (int)(r % D);
    const long long n = r / D;
    int zl, zh, yl, yh, xl, xh;
    ac_range(z, rz, Do, zl, zh);
    ac_range(y, ry, Ho, yl, yh);
    ac_range(x, rx, Wo, xl, xh);
    float acc[8];
    T* p = g_in + ((((n * D + z) * H + y) * W + x) * (long long)C) + g * 8;
    if (accumulate) load8(p, acc);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    }
    for (int zo = zl; zo <= zh; ++zo) {
      const float wz = ac_weight(zo, z, rz, D);
      if (wz == 0.f) continue;
      for (int yo = yl; yo <= yh; ++yo) {
        const float wy = ac_weight(yo, y, ry, H);
        if (wy == 0.f) continue;
        for (int xo = xl; xo <= xh; ++xo) {
          const float wx = ac_weight(xo, x, rx, W);
          if (wx == 0.f) continue;
          float v[8];
          load8(g_out + ((((n * Do + zo) * Ho + yo) * Wo + xo) * (long long)C) + g * 8, v);
          const float w = wz * wy * wx;
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += w * v[j];
        }
      }
    }
    store8(p, acc);
  }
}

// Tiled, separable form of the same transposed interpolation (the form the network uses).  The gather above spends its
// time evaluating ~7^3 candidate weights and issuing up to 64 16-byte loads per lane.  The trilinear weight factorises,
// so a block first reduces z and y for the fine x-columns its coarse tile touches (<= 16 loads per item, coalesced
// along x and channels) into LDS, then reduces x from LDS (<= 4 reads per item): ~4x fewer L1 transactions and ~6x
// fewer weight evaluations, no temporary tensor in HBM.
constexpr int UB_TX = 16, UB_XF = 44;   // coarse x per block; fine x columns a tile can touch (2.0625 * 17 + 4 < 44)
template <typename T, int TY>
__global__ void __launch_bounds__(256)
upsample2_bwd_tiled_kernel(const T* __restrict__ g_out, int C, T* g_in, int accumulate, int D, int H, int W) {
  extern __shared__ __attribute__((aligned(16))) float us[];   // [TY][UB_XF][C]
  const int G = C / 8, Do = 2 * D, Ho = 2 * H, Wo = 2 * W;
  const float rz = ac_scale(D, Do), ry = ac_scale(H, Ho), rx = ac_scale(W, Wo);
  const int x0 = blockIdx.x * UB_TX, y0 = blockIdx.y * TY;
  const int z = blockIdx.z % D;
  const long long n = blockIdx.z / D;
  const int x1 = (x0 + UB_TX < W ? x0 + UB_TX : W) - 1;
  int xf0, xf1, t0, t1;
  ac_range(x0, rx, Wo, xf0, t0);
  ac_range(x1, rx, Wo, t1, xf1);
  const int nxf = xf1 - xf0 + 1;          // <= UB_XF (checked by the launcher's choice of UB_TX / UB_XF)
  int zl, zh;
  ac_range(z, rz, Do, zl, zh);
  // the z weights of the block's plane and the y weights of its TY rows, evaluated once (not per item and candidate)
  __shared__ float wzs[12], wys[TY][12];
  __shared__ int yls[TY], yhs[TY];
  if (threadIdx.x < 12) wzs[threadIdx.x] = (zl + (int)threadIdx.x <= zh) ? ac_weight(zl + (int)threadIdx.x, z, rz, D) : 0.f;
  if (threadIdx.x >= 64 && threadIdx.x < 64 + TY * 12) {
    const int yi = (threadIdx.x - 64) / 12, k = (threadIdx.x - 64) % 12, y = y0 + yi;
    int yl = 0, yh = -1;
    if (y < H) ac_range(y, ry, Ho, yl, yh);
    wys[yi][k] = (yl + k <= yh) ? ac_weight(yl + k, y, ry, H) : 0.f;
    if (k == 0) { yls[yi] = yl; yhs[yi] = yh < yl + 11 ? yh : yl + 11; }
  }
  __syncthreads();
  const int zh_c = zh < zl + 11 ? zh : zl + 11;   // (the candidate range is at most 9 wide)
  // phase 1: reduce z and y
  for (int item = threadIdx.x; item < TY * nxf * G; item += 256) {
    const int g = item % G;
    int r = item / G;
    const int xi = r % nxf, yi = r / nxf;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    const int yl = yls[yi], yh = yhs[yi];
    for (int zo = zl; zo <= zh_c; ++zo) {
      const float wz = wzs[zo - zl];
      if (wz == 0.f) continue;
      for (int yo = yl; yo <= yh; ++yo) {
        const float wy = wys[yi][yo - yl];
        if (wy == 0.f) continue;
        float v[8];
        load8(g_out + ((((n * Do + zo) * Ho + yo) * Wo + (xf0 + xi)) * (long long)C) + g * 8, v);
        const float w = wz * wy;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += w * v[j];
      }
    }
    float* q = us + (yi * UB_XF + xi) * C + g * 8;
    store8(q, acc);
  }
  __syncthreads();
  // phase 2: reduce x
  for (int item = threadIdx.x; item < TY * UB_TX * G; item += 256) {
    const int g = item % G;
    int r = item / G;
    const int xi = r % UB_TX, yi = r / UB_TX;
    const int x = x0 + xi, y = y0 + yi;
    if (x >= W || y >= H) continue;
    int xl, xh;
    ac_range(x, rx, Wo, xl, xh);
    T* p = g_in + ((((n * D + z) * H + y) * W + x) * (long long)C) + g * 8;
    float acc[8];
    if (accumulate) load8(p, acc);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    }
    for (int xo = xl; xo <= xh; ++xo) {
      const float wx = ac_weight(xo, x, rx, W);
      if (wx == 0.f) continue;
      const float* q = us + (yi * UB_XF + (xo - xf0)) * C + g * 8;
      const float4 a = reinterpret_cast<const float4*>(q)[0], b = reinterpret_cast<const float4*>(q)[1];
      acc[0] += wx * a.x; acc[1] += wx * a.y; acc[2] += wx * a.z; acc[3] += wx * a.w;
      acc[4] += wx * b.x; acc[5] += wx * b.y; acc[6] += wx * b.z; acc[7] += wx * b.w;
    }
    store8(p, acc);
  }
}

// z-marching form of the tiled kernel (the one the network uses when every coarse extent is >= 4).  The tiled kernel
// above gives each coarse plane its own block, so every fine plane is fetched by the ~2 coarse planes it feeds and the
// interpolation ranges are re-derived per block.  Here a block owns TY x 16 coarse (y, x) positions and a run of ZS
// coarse planes and walks the fine planes under it ONCE, in order: a fine plane is reduced over y (global loads -> LDS)
// and x (LDS -> registers) to the block's coarse footprint, and that partial is added to the two coarse planes it feeds
// (weights 1-lam / lam of ac_src), held in two rotating register accumulators; a coarse plane is stored when the walk
// has passed it.  Every range and weight is evaluated once per block.
constexpr int UM_TX = 16, UM_XF = 40, UM_K = 6;   // coarse x per block; fine x columns under them; candidates per coarse index
__device__ __forceinline__ void ac_exact(int i, float rs, int in, int out, int& lo, int& n, float (&w)[UM_K]) {
  // the contiguous fine indices o with ac_src(o).i0 == i or .i1 == i, and their weights (<= 5 for in >= 4)
  int l, h;
  ac_range(i, rs, out, l, h);
  int i0, i1; float lam;
  for (;; ++l) { ac_src(l, rs, in, i0, i1, lam); if (i1 >= i || l >= h) break; }
  for (;; --h) { ac_src(h, rs, in, i0, i1, lam); if (i0 <= i || h <= l) break; }
  lo = l;
  n = h - l + 1 < UM_K ? h - l + 1 : UM_K;
#pragma unroll
  for (int k = 0; k < UM_K; ++k) w[k] = k < n ? ac_weight(l + k, i, rs, in) : 0.f;
}
template <typename T, int TY>
__global__ void __launch_bounds__(256, 2)
upsample2_bwd_march_kernel(const T* __restrict__ g_out, int C, T* g_in, int accumulate, int D, int H, int W, int ZS) {
  extern __shared__ __attribute__((aligned(16))) float us[];   // [2][TY][UM_XF][C]: one buffer per fine plane, alternating
  __shared__ float wys[TY][UM_K];
  __shared__ int yls[TY], nys[TY];
  const int G = C / 8, Do = 2 * D, Ho = 2 * H, Wo = 2 * W;
  const float rz = ac_scale(D, Do), ry = ac_scale(H, Ho), rx = ac_scale(W, Wo);
  const TileIdx3 tl = xcd_contiguous_tile3();                  // (round 4: neighbouring tiles on one XCD, the halo in one L2)
  const int x0 = tl.x * UM_TX, y0 = tl.y * TY;
  const int nseg = (D + ZS - 1) / ZS;
  const int seg = tl.z % nseg;
  const long long n = tl.z / nseg;
  const int zc0 = seg * ZS, zc1 = zc0 + ZS < D ? zc0 + ZS : D;
  const int x1 = (x0 + UM_TX < W ? x0 + UM_TX : W) - 1;
  int i0, i1; float lam;
  // fine x columns / fine planes that feed this block (exact: first index whose upper target reaches the block, last whose
  // lower target is still inside)
  int xf0, xf1, t;
  ac_range(x0, rx, Wo, xf0, t);
  for (;; ++xf0) { ac_src(xf0, rx, W, i0, i1, lam); if (i1 >= x0 || xf0 >= Wo - 1) break; }
  ac_range(x1, rx, Wo, t, xf1);
  for (;; --xf1) { ac_src(xf1, rx, W, i0, i1, lam); if (i0 <= x1 || xf1 <= xf0) break; }
  const int nxf = xf1 - xf0 + 1 < UM_XF ? xf1 - xf0 + 1 : UM_XF;
  int zf0, zf1;
  ac_range(zc0, rz, Do, zf0, t);
  for (;; ++zf0) { ac_src(zf0, rz, D, i0, i1, lam); if (i1 >= zc0 || zf0 >= Do - 1) break; }
  ac_range(zc1 - 1, rz, Do, t, zf1);
  for (;; --zf1) { ac_src(zf1, rz, D, i0, i1, lam); if (i0 <= zc1 - 1 || zf1 <= zf0) break; }
  if (threadIdx.x < TY) {
    const int y = y0 + (int)threadIdx.x;
    float w[UM_K];
    int lo = 0, cnt = 0;
    if (y < H) ac_exact(y, ry, H, Ho, lo, cnt, w);
    yls[threadIdx.x] = lo; nys[threadIdx.x] = cnt;
#pragma unroll
    for (int k = 0; k < UM_K; ++k) wys[threadIdx.x][k] = (y < H && k < cnt) ? w[k] : 0.f;
  }
  // this thread's two phase-2 items (coarse y, coarse x, 8 channels): x range and weights, output pointer
  constexpr int NI = 1;     // TY * 16 * G = 256 items
  float wx[NI][UM_K];
  int xrel[NI], qoff[NI];
  bool live[NI];
  long long pofs[NI];
#pragma unroll
  for (int it = 0; it < NI; ++it) {
    const int item = threadIdx.x + 256 * it;
    const int g = item % G;
    const int r = item / G;
    const int xi = r % UM_TX, yi = r / UM_TX;
    const int x = x0 + xi, y = y0 + yi;
    live[it] = yi < TY && x < W && y < H;
    int lo = xf0, cnt = 0;
    if (live[it]) ac_exact(x, rx, W, Wo, lo, cnt, wx[it]);
    else {
#pragma unroll
      for (int k = 0; k < UM_K; ++k) wx[it][k] = 0.f;
    }
    // columns beyond the staged range carry zero weight; clamp the window into the stage so every read stays inside it
    xrel[it] = lo - xf0;
    if (xrel[it] < 0) xrel[it] = 0;
    if (xrel[it] > UM_XF - UM_K) xrel[it] = UM_XF - UM_K;
    if (live[it] && xrel[it] != lo - xf0) {   // re-derive the weights for the clamped window (border tiles only)
#pragma unroll
      for (int k = 0; k < UM_K; ++k) wx[it][k] = ac_weight(xf0 + xrel[it] + k, x, rx, W);
    }
    qoff[it] = ((yi < TY ? yi : 0) * UM_XF + xrel[it]) * C + g * 8;
    pofs[it] = (((n * D) * H + y) * (long long)W + x) * C + g * 8;   // + z * H * W * C
  }
  float accA[NI][8], accB[NI][8];
#pragma unroll
  for (int it = 0; it < NI; ++it)
#pragma unroll
    for (int j = 0; j < 8; ++j) { accA[it][j] = 0.f; accB[it][j] = 0.f; }
  ac_src(zf0, rz, D, i0, i1, lam);
  int cur = i0;                                   // accA <-> coarse plane cur, accB <-> cur + 1
  const long long plane = (long long)H * W * C;
  auto flush = [&](int z, float (&acc)[NI][8]) {
    if (z < zc0 || z >= zc1) return;
#pragma unroll
    for (int it = 0; it < NI; ++it) {
      if (!live[it]) continue;
      T* p = g_in + pofs[it] + z * plane;
      float o[8];
      if (accumulate) {
        load8(p, o);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] += acc[it][j];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = acc[it][j];
      }
      store8(p, o);
    }
  };
  __syncthreads();
  // phase-1 items of this thread (coarse row, fine column, 8 channels), fixed for the whole walk: TY * G = 16, so
  // TY * nxf * G <= 640 -> 3 per thread
  constexpr int N1 = 3, KY = 5;
  int gofs[N1];           // element offset of the item's first fine row inside a fine plane (< 2^31: checked by the launcher); < 0: no item
  int uofs[N1], ycnt[N1], yrow[N1];
#pragma unroll
  for (int it = 0; it < N1; ++it) {
    const int item = threadIdx.x + 256 * it;
    const int g = item % G;
    const int r = item / G;
    const int xi = r % nxf, yi = r / nxf;
    const bool on = item < TY * nxf * G;
    const int yy = on ? yi : 0;
    gofs[it] = on ? (yls[yy] * Wo + (xf0 + xi)) * C + g * 8 : -1;
    uofs[it] = (yy * UM_XF + xi) * C + g * 8;
    ycnt[it] = on ? (nys[yy] < KY ? nys[yy] : KY) : 0;
    yrow[it] = yy;
  }
  Pack8<T> raw[N1][KY];
  auto issue = [&](int zo) {
    const T* gz = g_out + ((n * Do + zo) * (long long)Ho) * Wo * C;
#pragma unroll
    for (int it = 0; it < N1; ++it)
#pragma unroll
      for (int k = 0; k < KY; ++k)
        if (k < ycnt[it])   // uniform base + 32-bit byte offset: one address register per load, not a 64-bit pair
          load8p(reinterpret_cast<const T*>(reinterpret_cast<const char*>(gz) + (unsigned)((gofs[it] + k * Wo * C) * (int)sizeof(T))), raw[it][k]);
  };
  issue(zf0);
  int buf = 0;
  for (int zo = zf0; zo <= zf1; ++zo) {
    ac_src(zo, rz, D, i0, i1, lam);
    if (i0 > cur) {                               // (the source index advances by at most one per fine plane: scale < 1)
      flush(cur, accA);
#pragma unroll
      for (int it = 0; it < NI; ++it)
#pragma unroll
        for (int j = 0; j < 8; ++j) { accA[it][j] = accB[it][j]; accB[it][j] = 0.f; }
      cur = i0;
    }
    const float wA = (1.f - lam) + (i1 == i0 ? lam : 0.f), wB = i1 != i0 ? lam : 0.f;
    // phase 1: the fetched rows of fine plane zo reduced over y into this plane's LDS buffer
    float* ub = us + buf * (TY * UM_XF * C);
#pragma unroll
    for (int it = 0; it < N1; ++it) {
      if (gofs[it] < 0) continue;
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
      for (int k = 0; k < KY; ++k) {
        if (k < ycnt[it]) {
          float v[8];
          unpack8(raw[it][k], v);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += wys[yrow[it]][k] * v[j];
        }
      }
      float* q = ub + uofs[it];
      store8(q, acc);
    }
    __syncthreads();     // the one barrier per fine plane: the buffers alternate, so plane zo + 2 overwrites this one only
                         // after every thread has passed the barrier of plane zo + 1, i.e. finished reading it
    if (zo < zf1) issue(zo + 1);   // in flight during phase 2
    // phase 2: reduce x from LDS, add to the two coarse planes this fine plane feeds
#pragma unroll
    for (int it = 0; it < NI; ++it) {
      float pz[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) pz[j] = 0.f;
#pragma unroll
      for (int k = 0; k < UM_K; ++k) {
        const float w = wx[it][k];
        if (xrel[it] + k < nxf) {
          const float* q = ub + qoff[it] + k * C;
          const float4 a = reinterpret_cast<const float4*>(q)[0], b = reinterpret_cast<const float4*>(q)[1];
          pz[0] += w * a.x; pz[1] += w * a.y; pz[2] += w * a.z; pz[3] += w * a.w;
          pz[4] += w * b.x; pz[5] += w * b.y; pz[6] += w * b.z; pz[7] += w * b.w;
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) { accA[it][j] += wA * pz[j]; accB[it][j] += wB * pz[j]; }
    }
    buf ^= 1;
  }
  flush(cur, accA);
  flush(cur + 1, accB);
}

// ---------------- routes and launchers --------------------------------------------------------------
// The launch cut of one pass: which of the three forms runs, with which grid, dynamic LDS and form parameters.  The launchers
// and upsample2_form() take it from upsample2_fwd_cut() / upsample2_bwd_cut(); a launch follows from the cut alone.
enum class Up2Form { Gather = 0, Tiled = 1, March = 2 };
struct Up2Cut {
  Up2Form form;
  dim3 grid;
  size_t lds;         // dynamic LDS bytes
  int lds_limit;      // > 0: the kernel's dynamic-LDS limit is set to this before the launch
  int XF;             // forward march: fine columns per block
  int TY, ZS, nseg;   // backward: coarse rows per block (tiled, march); coarse planes per z segment, segments per sample (march)
  long long total;    // gather: (voxel, 8 channels) items
};
static Up2Cut upsample2_gather_cut(long long total) {
  Up2Cut c{};
  c.form = Up2Form::Gather; c.total = total; c.grid = dim3((unsigned)grid_for(total));
  return c;
}
static Up2Cut upsample2_fwd_cut(int dtype, int C, Dims d) {
  Up2Cut c{};
  if ((C == 32 || C == 64 || C == 128) && d.D >= 2 && d.H >= 2 && d.W >= 2) {
    c.XF = 4096 / C;                                       // fine columns per block: four (row, column, 8-channel) items per thread
    const int nseg = (2 * d.D + UFM_ZSF - 1) / UFM_ZSF;
    c.lds = (size_t)2 * 3 * UFM_XC * C * dtype_size(dtype);   // <= 102 KB except 128 channels in f32 (tiled kernel)
    if ((long long)d.N * nseg <= 65535 && d.H <= 65535 && c.lds <= 112 * 1024) {
      c.form = Up2Form::March; c.lds_limit = c.lds > 48 * 1024 ? 112 * 1024 : 0;
      c.grid = dim3((unsigned)((2 * d.W + c.XF - 1) / c.XF), (unsigned)d.H, (unsigned)(d.N * nseg));
      return c;
    }
  }
  c = Up2Cut{};
  c.lds = (size_t)4 * UF_XC * C * sizeof(float);
  if (c.lds <= 144 * 1024 && (long long)d.N * d.D <= 65535 && d.H <= 65535) {   // up to 128 channels
    c.form = Up2Form::Tiled; c.lds_limit = c.lds > 48 * 1024 ? 144 * 1024 : 0;
    c.grid = dim3((unsigned)((2 * d.W + UF_XF - 1) / UF_XF), (unsigned)d.H, (unsigned)((long long)d.N * d.D));
    return c;
  }
  return upsample2_gather_cut((long long)d.N * d.vox() * 8 * (C / 8));
}
static Up2Cut upsample2_bwd_cut(int dtype, int C, Dims d) {
  Up2Cut c{};
  // z-marching kernel: TY * C = 128 (256 phase-2 items of 8 channels = 1 per thread), LDS = 2 x 128 * 40 floats = 40 KB
  // (16-bit storage only: the f32 parity mode would hold 200 registers of fetched rows; it stays on the tiled kernel; a
  // thread reaches the rows of a fine plane through 32-bit offsets)
  if (dtype_size(dtype) == 2 && (C == 32 || C == 64 || C == 128) && d.D >= 4 && d.H >= 4 && d.W >= 4 &&
      (long long)4 * d.H * d.W * C < (1LL << 31)) {
    c.form = Up2Form::March; c.TY = 128 / C; c.ZS = d.D >= 32 ? 8 : 4; c.nseg = (d.D + c.ZS - 1) / c.ZS;
    c.lds = (size_t)2 * 128 * UM_XF * sizeof(float);   // 40 KB: four workgroups per CU
    c.lds_limit = (int)c.lds;
    c.grid = dim3((unsigned)((d.W + UM_TX - 1) / UM_TX), (unsigned)((d.H + c.TY - 1) / c.TY), (unsigned)(d.N * c.nseg));
    return c;
  }
  // tiled separable kernel: LDS = TY * 44 * C floats <= 45 KB with TY = 4 up to 64 channels, TY = 2 up to 128
  if (C <= 128 && (long long)d.N * d.D <= 65535 && d.W >= 2) {
    c.form = Up2Form::Tiled; c.TY = C <= 64 ? 4 : 2; c.lds = (size_t)c.TY * UB_XF * C * sizeof(float);
    c.grid = dim3((unsigned)((d.W + UB_TX - 1) / UB_TX), (unsigned)((d.H + c.TY - 1) / c.TY), (unsigned)((long long)d.N * d.D));
    return c;
  }
  return upsample2_gather_cut((long long)d.N * d.vox() * (C / 8));
}
// diagnostic: the form of a pass (0 gather, 1 tiled, 2 march), so that a host test can pin the route
int upsample2_form(int dtype, int C, Dims d, bool backward) {
  return (int)(backward ? upsample2_bwd_cut(dtype, C, d) : upsample2_fwd_cut(dtype, C, d)).form;
}

template <auto KERNEL>
static int upsample2_lds_limit(const Up2Cut& c) {   // once per kernel instantiation and device
  static unsigned long long configured = 0;
  return c.lds_limit ? configure_kernel_lds(configured, reinterpret_cast<const void*>(KERNEL), c.lds_limit) : 0;
}
template <typename T>
static int upsample2_fwd_run(const Up2Cut& c, const T* in, int C, T* out, Dims d, hipStream_t s) {
  if (c.form == Up2Form::March) {
    if (int e = upsample2_lds_limit<&upsample2_fwd_march_kernel<T>>(c)) return e;
    upsample2_fwd_march_kernel<T><<<c.grid, 256, c.lds, s>>>(in, C, out, d.D, d.H, d.W, c.XF);
  } else if (c.form == Up2Form::Tiled) {
    if (int e = upsample2_lds_limit<&upsample2_fwd_tiled_kernel<T>>(c)) return e;
    upsample2_fwd_tiled_kernel<T><<<c.grid, 256, c.lds, s>>>(in, C, out, d.D, d.H, d.W);
  } else {
    upsample2_fwd_kernel<T><<<c.grid, 256, 0, s>>>(in, C, out, d.D, d.H, d.W, c.total);
  }
  SEUNET_LAUNCH_CHECK();
  return 0;
}
int launch_upsample2_fwd(int dtype, const void* in, int C, void* out, Dims d, hipStream_t s) {
  SEUNET_CHECK(C % 8 == 0, "upsample2: C=%d must be a multiple of 8", C);
  const Up2Cut cut = upsample2_fwd_cut(dtype, C, d);
  int e = -1;
  SEUNET_DTYPE_SWITCH(dtype, e = upsample2_fwd_run<T>(cut, (const T*)in, C, (T*)out, d, s));
  return e;
}

template <typename T, int TY>
static int upsample2_bwd_march_run(const Up2Cut& c, const T* g_out, int C, T* g_in, int accumulate, Dims d, hipStream_t s) {
  if (int e = upsample2_lds_limit<&upsample2_bwd_march_kernel<T, TY>>(c)) return e;
  upsample2_bwd_march_kernel<T, TY><<<c.grid, 256, c.lds, s>>>(g_out, C, g_in, accumulate, d.D, d.H, d.W, c.ZS);
  return 0;
}
template <typename T>
static int upsample2_bwd_run(const Up2Cut& c, const T* g_out, int C, T* g_in, int accumulate, Dims d, hipStream_t s) {
  if (c.form == Up2Form::March) {
    int e = -1;
    if constexpr (sizeof(T) == 2)
      e = c.TY == 4 ? upsample2_bwd_march_run<T, 4>(c, g_out, C, g_in, accumulate, d, s)
        : c.TY == 2 ? upsample2_bwd_march_run<T, 2>(c, g_out, C, g_in, accumulate, d, s)
                    : upsample2_bwd_march_run<T, 1>(c, g_out, C, g_in, accumulate, d, s);
    if (e) return e;
  } else if (c.form == Up2Form::Tiled) {
    if (c.TY == 4) upsample2_bwd_tiled_kernel<T, 4><<<c.grid, 256, c.lds, s>>>(g_out, C, g_in, accumulate, d.D, d.H, d.W);
    else upsample2_bwd_tiled_kernel<T, 2><<<c.grid, 256, c.lds, s>>>(g_out, C, g_in, accumulate, d.D, d.H, d.W);
  } else {
    upsample2_bwd_kernel<T><<<c.grid, 256, 0, s>>>(g_out, C, g_in, accumulate, d.D, d.H, d.W, c.total);
  }
  SEUNET_LAUNCH_CHECK();
  return 0;
}
int launch_upsample2_bwd(int dtype, const void* g_out, int C, void* g_in, int accumulate, Dims d,
                         hipStream_t s) {
  SEUNET_CHECK(C % 8 == 0, "upsample2: C=%d must be a multiple of 8", C);
  const Up2Cut cut = upsample2_bwd_cut(dtype, C, d);
  SEUNET_CHECK(cut.form != Up2Form::March || (long long)d.N * cut.nseg <= 65535, "upsample2_bwd: batch too large");
  int e = -1;
  SEUNET_DTYPE_SWITCH(dtype, e = upsample2_bwd_run<T>(cut, (const T*)g_out, C, (T*)g_in, accumulate, d, s));
  return e;
}

}  // namespace seunet
