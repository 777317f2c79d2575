// The two deep-supervision heads and the side-map up-sampling (gfx950).  All HBM-bound.
//
//   side maps     the per-block side-map up-sampling by 1/2/4/8 (reference SE_UNet.py:19,34,61,81)
//   heads         reference SE_UNet.py:150-153,232-233: 1x1x1 conv over the DropLayer-scaled stack of
//                 up-sampled side maps.  Both are linear, so the head weight and the DropLayer scale
//                 are applied to each side map at its native resolution (gate.hip accumulates a
//                 single-channel "level map" per resolution) and only those maps are interpolated.
#include "seunet_common.h"
#include "trilinear.h"

namespace seunet {

// ---------------- side map up-sampling to NCDHW (block-level API / tests only) ------------------
__global__ void side_upsample_kernel(const float* __restrict__ side, int C, int scale,
                                     float* __restrict__ out, int c_total, int c_off, int D, int H, int W,
                                     long long total) {
  const int Do = D * scale, Ho = H * scale, Wo = W * scale;
  const float rz = ac_scale(D, Do), ry = ac_scale(H, Ho), rx = ac_scale(W, Wo);
  const long long Vo = (long long)Do * Ho * Wo;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    long long r = i;
    const int xo = (int)(r % Wo); r /= Wo;
    const int yo = (int)(r % Ho); r /= Ho;
    const int zo = (int)(r % Do);
    const long long n = r / Do;
    int z0, z1, y0, y1, x0, x1; float lz, ly, lx;
    ac_src(zo, rz, D, z0, z1, lz);
    ac_src(yo, ry, H, y0, y1, ly);
    ac_src(xo, rx, W, x0, x1, lx);
    for (int c = 0; c < C; ++c) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int z = (k & 4) ? z1 : z0, y = (k & 2) ? y1 : y0, x = (k & 1) ? x1 : x0;
        const float w = ((k & 4) ? lz : 1.f - lz) * ((k & 2) ? ly : 1.f - ly) * ((k & 1) ? lx : 1.f - lx);
        acc += w * side[((((n * D + z) * H + y) * W + x) * (long long)C) + c];
      }
      out[(n * c_total + c_off + c) * Vo + (((long long)zo * Ho + yo) * Wo + xo)] = acc;
    }
  }
}

// ---------------- heads ---------------------------------------------------------------------------
struct HeadLevels {
  const float* map[4];  // level l has extents (D0>>l, H0>>l, W0>>l); null = level absent
};

// One thread = 4 consecutive x of one (n, z, y) row: the z / y source rows and weights of every level are shared by the
// four outputs (the per-voxel form spent ~260 vector instructions per voxel, 87 us per head at 4x128^3).
__global__ void __launch_bounds__(256)
head_fwd_kernel(HeadLevels lv, const float* __restrict__ bias, float* __restrict__ pred,
                int D, int H, int W, long long total4) {
  const int W4 = W >> 2;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total4;
       i += (long long)gridDim.x * blockDim.x) {
    long long r = i;
    const int xq = (int)(r % W4); r /= W4;
    const int yo = (int)(r % H); r /= H;
    const int zo = (int)(r % D);
    const long long n = r / D;
    const long long o = ((n * D + zo) * H + yo) * (long long)W + 4 * xq;
    float acc[4];
    const float b0 = bias[0];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = b0;
    if (lv.map[0]) {
      const float4 v = *reinterpret_cast<const float4*>(lv.map[0] + o);
      acc[0] += v.x; acc[1] += v.y; acc[2] += v.z; acc[3] += v.w;
    }
#pragma unroll
    for (int l = 1; l < 4; ++l) {
      if (!lv.map[l]) continue;
      const int Dl = D >> l, Hl = H >> l, Wl = W >> l;
      int z0, z1, y0, y1; float lz, ly;
      ac_src(zo, ac_scale(Dl, D), Dl, z0, z1, lz);
      ac_src(yo, ac_scale(Hl, H), Hl, y0, y1, ly);
      const float* m = lv.map[l] + n * (long long)Dl * Hl * Wl;
      const float* r00 = m + ((long long)z0 * Hl + y0) * Wl;
      const float* r01 = m + ((long long)z0 * Hl + y1) * Wl;
      const float* r10 = m + ((long long)z1 * Hl + y0) * Wl;
      const float* r11 = m + ((long long)z1 * Hl + y1) * Wl;
      const float w00 = (1.f - lz) * (1.f - ly), w01 = (1.f - lz) * ly, w10 = lz * (1.f - ly), w11 = lz * ly;
      const float rx = ac_scale(Wl, W);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int x0, x1; float lx;
        ac_src(4 * xq + k, rx, Wl, x0, x1, lx);
        // same association as the 8-corner sum: (wz*wy)*wx per corner
        const float a0 = w00 * r00[x0] + w01 * r01[x0] + w10 * r10[x0] + w11 * r11[x0];
        const float a1 = w00 * r00[x1] + w01 * r01[x1] + w10 * r10[x1] + w11 * r11[x1];
        acc[k] += (1.f - lx) * a0 + lx * a1;
      }
    }
    *reinterpret_cast<float4*>(pred + o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  }
}
// Row form of the same head: a block per (n, z) plane, ONE WAVE per output row.  The per-voxel form above issues 8 four-byte
// gathers per level and output and decodes its 64-bit flat index per thread (~400 vector instructions per 4 voxels: 62 us per
// head at 4 x 128^3 against 12 us of HBM time).  Here everything that depends on (n, z, y) only is wave-uniform (scalar
// registers); the lanes first blend the four (z, y) source rows of a level with coalesced loads -- c[xc] = w00 r00[xc] + w01
// r01[xc] + w10 r10[xc] + w11 r11[xc], W >> l values -- into a per-wave LDS row, then every lane interpolates its outputs along
// x from that row with x indices / weights tabulated once per thread.  Same products and association as head_fwd_kernel.
constexpr int HF_RPW = 4;     // rows per wave: their loads are issued together (a wave that walks its rows one by one is a
                              // chain of dependent global load -> LDS -> read -> store latencies)
__global__ void __launch_bounds__(256)
head_fwd_rows_kernel(HeadLevels lv, const float* __restrict__ bias, float* __restrict__ pred, int D, int H, int W) {
  extern __shared__ float hrow[];                       // [4 waves][HF_RPW rows][W/2 + W/4 + W/8]
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int per_row = (W >> 1) + (W >> 2) + (W >> 3);
  float* const rb = hrow + wv * HF_RPW * per_row;
  const float b0 = bias[0];
  const int ybl = (H + 4 * HF_RPW - 1) / (4 * HF_RPW);           // y blocks per plane
  const int yb = blockIdx.x % ybl, zo = (blockIdx.x / ybl) % D, n = blockIdx.x / (ybl * D);
  const int ybase = (yb * 4 + wv) * HF_RPW;
  // the level-0 values of the first pass over x (requested first: they arrive while the coarse rows are blended)
  float2 v0[HF_RPW];
#pragma unroll
  for (int r = 0; r < HF_RPW; ++r) {
    const int yo = ybase + r < H ? ybase + r : H - 1;
    v0[r] = (lv.map[0] && 2 * lane < W) ? *reinterpret_cast<const float2*>(lv.map[0] + (((long long)n * D + zo) * H + yo) * W + 2 * lane)
                                        : make_float2(0.f, 0.f);
  }
  // x tables of this lane's first two outputs (x = 2 lane, 2 lane + 1); further passes (W > 128) recompute
  int tx0[3][2], tx1[3][2]; float tlx[3][2];
#pragma unroll
  for (int l = 1; l < 4; ++l)
#pragma unroll
    for (int k = 0; k < 2; ++k) ac_src(2 * lane + k, ac_scale(W >> l, W), W >> l, tx0[l - 1][k], tx1[l - 1][k], tlx[l - 1][k]);
#pragma unroll
  for (int l = 1; l < 4; ++l) {
    if (!lv.map[l]) continue;
    const int Dl = D >> l, Hl = H >> l, Wl = W >> l;
    int z0, z1; float lz;
    ac_src(zo, ac_scale(Dl, D), Dl, z0, z1, lz);
    const float* m = lv.map[l] + (long long)n * Dl * Hl * Wl;
    const int lbase = (l > 1 ? (W >> 1) : 0) + (l > 2 ? (W >> 2) : 0);
#pragma unroll
    for (int r = 0; r < HF_RPW; ++r) {
      const int yo = ybase + r < H ? ybase + r : H - 1;
      int y0, y1; float ly;
      ac_src(yo, ac_scale(Hl, H), Hl, y0, y1, ly);
      const float* r00 = m + (z0 * Hl + y0) * Wl;
      const float* r01 = m + (z0 * Hl + y1) * Wl;
      const float* r10 = m + (z1 * Hl + y0) * Wl;
      const float* r11 = m + (z1 * Hl + y1) * Wl;
      const float w00 = (1.f - lz) * (1.f - ly), w01 = (1.f - lz) * ly, w10 = lz * (1.f - ly), w11 = lz * ly;
      for (int xc = lane; xc < Wl; xc += 64)
        rb[r * per_row + lbase + xc] = w00 * r00[xc] + w01 * r01[xc] + w10 * r10[xc] + w11 * r11[xc];
    }
  }
  __builtin_amdgcn_wave_barrier();                      // LDS operations of one wave complete in order
#pragma unroll
  for (int r = 0; r < HF_RPW; ++r) {
    const int yo = ybase + r;
    if (yo >= H) break;                                 // (wave-uniform)
    const long long orow = (((long long)n * D + zo) * H + yo) * W;
    for (int x = 2 * lane; x < W; x += 128) {
      float acc[2] = {b0, b0};
      if (lv.map[0]) {
        const float2 v = x < 128 ? v0[r] : *reinterpret_cast<const float2*>(lv.map[0] + orow + x);
        acc[0] += v.x; acc[1] += v.y;
      }
      int lb = r * per_row;
#pragma unroll
      for (int l = 1; l < 4; ++l) {
        if (!lv.map[l]) continue;
        const int Wl = W >> l;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          int x0 = tx0[l - 1][k], x1 = tx1[l - 1][k]; float lx = tlx[l - 1][k];
          if (x >= 128) ac_src(x + k, ac_scale(Wl, W), Wl, x0, x1, lx);
          acc[k] += (1.f - lx) * rb[lb + x0] + lx * rb[lb + x1];
        }
        lb += Wl;
      }
      *reinterpret_cast<float2*>(pred + orow + x) = make_float2(acc[0], acc[1]);
    }
  }
}

// The x-axis pass of head_bwd for ALL levels of a head in one launch, plus the partial sums of the bias gradient: g_pred (the
// largest tensor on this path, 4 B per full-resolution voxel) is read once instead of once per level and once more for
// sum(g_pred).  The interpolation weights depend on the x index only: each block tabulates them once in LDS (range start
// + up to HB_K weights per output and level) and then streams HB_ROWS x-rows, one wave per row.  Same weights and the same
// summation order as the axis pass, up_transpose_axis_multi_kernel (bitwise identical results).
// HB_K: weights per table row, and the register taps of a lane's second entry (the level-3 ones, ~20 taps), read out of those rows
constexpr int HB_ROWS = 32, HB_K = 24, HB_PAD = 24, HB_KA = 8;
// A table row keeps HB_K weights and no more.  For every W <= 1024 that 2^l divides, an output of level l has at most 6 (l = 1),
// 12 (l = 2, W = 20) and 23 (l = 3, W = 24) taps after its leading zero weights; a width that 2^(nlevels - 1) does not divide can
// have more (W = 28 with 4 levels: 27), and launch_head_bwd refuses it (head_extents_check).  The enumeration is repeated in
// float32 on the host by tests/test_epilogue_ragged_host.py.
constexpr int HB_MAX_TAPS = 23;
static_assert(HB_K >= HB_MAX_TAPS, "a table row of head_bwd_x_multi_kernel must hold every tap of a level-3 output");
__global__ void __launch_bounds__(256)
head_bwd_x_multi_kernel(const float* __restrict__ g, float* __restrict__ t1a, float* __restrict__ t1b, float* __restrict__ t1c,
                        int nl, int W, long long rows, double* __restrict__ bias_part) {
  extern __shared__ float hsm[];                        // [4][W + HB_PAD] row buffers (pad = zeros), then per output the table: lo, n, HB_K weights
  const int RW = W + HB_PAD;
  float* tab = hsm + 4 * RW;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long row0 = (long long)blockIdx.x * HB_ROWS;
  // rows of up to 256 values: ALL HB_ROWS / 4 rows of this wave are requested up front (registers), before the weight
  // table is built: with one row in flight
  // per wave the kernel moved 0.9 TB/s (bytes in flight x waves / HBM latency), not the table look-ups' fault
  constexpr int RPW = HB_ROWS / 4;
  const bool pf = W <= 256;
  float pre[RPW][4];
  if (pf) {
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
      const long long row = row0 + wv + 4 * j;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int x = lane + 64 * k;
        pre[j][k] = (row < rows && x < W) ? g[row * W + x] : 0.f;
      }
    }
  }
  float* const outs[3] = {t1a, t1b, t1c};
  // table: outputs of level l occupy entries [ebase_l, ebase_l + W >> l)
  int ebase[4] = {0, 0, W >> 1, (W >> 1) + (W >> 2)};
  const int nent = (nl > 1 ? W >> 1 : 0) + (nl > 2 ? W >> 2 : 0) + (nl > 3 ? W >> 3 : 0);
  for (int e = threadIdx.x; e < nent; e += 256) {
    const int l = e < ebase[2] ? 1 : (e < ebase[3] ? 2 : 3);
    const int i = e - ebase[l], Wl = W >> l;
    const float rs = ac_scale(Wl, W);
    int lo, hi;
    ac_range(i, rs, W, lo, hi);
    float* t = tab + e * (HB_K + 2);
    int cnt = 0, first = lo;
    bool started = false;
    for (int o = lo; o <= hi; ++o) {
      const float w = ac_weight(o, i, rs, Wl);
      if (!started && w == 0.f) { first = o + 1; continue; }     // leading zero weights: skipped exactly like `if (w != 0)`
      started = true;
      if (cnt < HB_K) t[2 + cnt] = w;
      ++cnt;
    }
    t[0] = __int_as_float(first);
    t[1] = __int_as_float(cnt < HB_K ? cnt : HB_K);
  }
  for (int i = threadIdx.x; i < 4 * HB_PAD; i += 256) hsm[(i / HB_PAD) * RW + W + i % HB_PAD] = 0.f;
  __syncthreads();
  // Fast path (<= 128 entries, i.e. W <= 146): a lane owns the same two entries (lane, lane + 64) in every row, so their taps
  // live in REGISTERS for the whole block -- the per-row work is then 30-odd LDS reads and FMAs instead of table look-ups.
  // (Measured by elimination at 4 x 128^3: row loads + LDS writes + bias sums 12.8 us, weight table 5 us, taps + stores 21 us;
  // the taps are unbalanced -- 16 lanes carry the ~20-tap level-3 entries -- which is what is left to fix.)  Taps beyond an entry's count carry
  // weight 0 and read the zero pad behind the row; skipping a zero weight and adding 0 * v give the same bits.
  const int e0 = lane, e1 = lane + 64;
  float wa[HB_KA], wb[HB_K];
  int fa = 0, fb = 0, ca = 0, cb = 0;
  {
    if (e0 < nent) { const float* t = tab + e0 * (HB_K + 2); fa = __float_as_int(t[0]); ca = __float_as_int(t[1]); }
    if (e1 < nent) { const float* t = tab + e1 * (HB_K + 2); fb = __float_as_int(t[0]); cb = __float_as_int(t[1]); }
#pragma unroll
    for (int k = 0; k < HB_KA; ++k) wa[k] = (e0 < nent && k < ca) ? tab[e0 * (HB_K + 2) + 2 + k] : 0.f;
#pragma unroll
    for (int k = 0; k < HB_K; ++k) wb[k] = (e1 < nent && k < cb) ? tab[e1 * (HB_K + 2) + 2 + k] : 0.f;
  }
  const bool fast = nent <= 128 && __all(ca <= HB_KA && cb <= HB_K && fa + HB_KA <= RW && fb + HB_K <= RW);   // (wave-uniform)
  int ka = 0, kb = 0;                                    // taps to walk: the wave's maxima, rounded up to 4
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { ca = max(ca, shfl_xor_settled(ca, off)); cb = max(cb, shfl_xor_settled(cb, off)); }
  ka = (ca + 3) & ~3; kb = (cb + 3) & ~3;
  const int la = e0 < ebase[2] ? 1 : (e0 < ebase[3] ? 2 : 3), lb = e1 < ebase[2] ? 1 : (e1 < ebase[3] ? 2 : 3);
  float* const outa = e0 < nent ? (la == 1 ? t1a : (la == 2 ? t1b : t1c)) : nullptr;
  float* const outb = e1 < nent ? (lb == 1 ? t1a : (lb == 2 ? t1b : t1c)) : nullptr;
  const int cola = e0 - ebase[la], colb = e1 - ebase[lb], wla = W >> la, wlb = W >> lb;
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < RPW; ++j) {
    const int rr = wv + 4 * j;
    const long long row = row0 + rr;
    if (row >= rows) break;                              // (wave-uniform)
    float* rb = hsm + wv * RW;
    if (pf) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int x = lane + 64 * k;
        if (x < W) { rb[x] = pre[j][k]; sum += (double)pre[j][k]; }
      }
    } else {
      for (int x = lane; x < W; x += 64) { const float v = g[row * W + x]; rb[x] = v; sum += (double)v; }
    }
    __builtin_amdgcn_wave_barrier();                     // LDS operations of one wave complete in order
    if (fast) {
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int k = 0; k < HB_KA; ++k)
        if (k < ka) a0 += wa[k] * rb[fa + k];
#pragma unroll
      for (int k = 0; k < HB_K; ++k)
        if (k < kb) a1 += wb[k] * rb[fb + k];
      if (outa) outa[row * wla + cola] = a0;
      if (outb) outb[row * wlb + colb] = a1;
      __builtin_amdgcn_wave_barrier();
      continue;
    }
    for (int e = lane; e < nent; e += 64) {
      const int l = e < ebase[2] ? 1 : (e < ebase[3] ? 2 : 3);
      float* out = outs[l - 1];
      if (out == nullptr) continue;
      const float* t = tab + e * (HB_K + 2);
      const int first = __float_as_int(t[0]), cnt = __float_as_int(t[1]);
      float acc = 0.f;
      for (int k = 0; k < cnt; k += 4) {                 // four taps at a time: independent LDS reads, same order of summation
        float w[4], v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool in = k + j < cnt;
          w[j] = in ? t[2 + k + j] : 0.f;
          v[j] = in ? rb[first + k + j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (w[j] != 0.f) acc += w[j] * v[j];
      }
      out[row * (W >> l) + (e - ebase[l])] = acc;
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (bias_part != nullptr) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += shfl_xor_settled(sum, off);
    __shared__ double wsum[4];
    if (lane == 0) wsum[wv] = sum;
    __syncthreads();
    if (threadIdx.x == 0) bias_part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  }
}

// deterministic sum of the f64 bias partials (fixed order: thread-strided sums, wave shuffles, 16 waves in order)
__global__ void __launch_bounds__(1024) sum_stage2_wide_kernel(const double* __restrict__ partial, int n, float* __restrict__ out) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) s += partial[i];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += shfl_xor_settled(s, off);
  __shared__ double w[16];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < 16; ++k) t += w[k];
    out[0] = (float)t;
  }
}

// The same sum by one 256-thread block, bit for bit: thread t stands for the four threads t, t + 256, t + 512, t + 768 of the
// 1024 (same lane, waves t / 64 + 4 j), so every thread-strided sum, every wave butterfly and the 16-wave order are the same.
__device__ __forceinline__ void sum_stage2_wide_by_256(const double* __restrict__ partial, int n, float* __restrict__ out) {
  __shared__ double w[16];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double s = 0.0;
    for (int i = threadIdx.x + 256 * j; i < n; i += 1024) s += partial[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += shfl_xor_settled(s, off);
    if ((threadIdx.x & 63) == 0) w[(threadIdx.x >> 6) + 4 * j] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < 16; ++k) t += w[k];
    out[0] = (float)t;
  }
}

// ---------------- launchers -----------------------------------------------------------------------
// Level l of a head has extents (D >> l, H >> l, W >> l) and is interpolated by exactly 2^l: every extent has to be a multiple
// of 2^(nlevels - 1).  (The x pass of the backward relies on it: see HB_K.)
static int head_extents_check(const char* what, Dims d0, int nlevels) {
  const int m = (1 << (nlevels - 1)) - 1;
  SEUNET_CHECK((d0.D & m) == 0 && (d0.H & m) == 0 && (d0.W & m) == 0,
               "%s: extents (%d, %d, %d) must be multiples of %d for %d levels", what, d0.D, d0.H, d0.W, m + 1, nlevels);
  return 0;
}

int launch_side_upsample(const float* side, int C, int scale, float* out, int c_total, int c_off, Dims dl,
                         hipStream_t s) {
  const long long total = (long long)dl.N * dl.vox() * scale * scale * scale;
  side_upsample_kernel<<<grid_for(total), 256, 0, s>>>(side, C, scale, out, c_total, c_off, dl.D, dl.H, dl.W, total);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_head_fwd(const float* const* level_maps, int nlevels, const float* bias, float* pred, Dims d0,
                    hipStream_t s) {
  SEUNET_CHECK(nlevels >= 1 && nlevels <= 4, "head: nlevels=%d out of range", nlevels);
  HeadLevels lv;
  for (int l = 0; l < 4; ++l) lv.map[l] = l < nlevels ? level_maps[l] : nullptr;
  for (int l = 1; l < nlevels; ++l)
    SEUNET_CHECK((d0.D >> l) >= 1 && (d0.H >> l) >= 1 && (d0.W >> l) >= 1, "head: volume too small for level %d", l);
  SEUNET_CHECK(d0.W % 4 == 0, "head: W=%d must be a multiple of 4", d0.W);
  if (int e = head_extents_check("head_fwd", d0, nlevels)) return e;
  if (d0.W % 8 == 0 && d0.W <= 2048 && (long long)d0.D * d0.H * d0.W < (1ll << 31)) {   // row form: whole level rows, LDS rows fit, 32-bit in-sample offsets
    const size_t lds = (size_t)4 * HF_RPW * ((d0.W >> 1) + (d0.W >> 2) + (d0.W >> 3)) * sizeof(float);
    const int ybl = (d0.H + 4 * HF_RPW - 1) / (4 * HF_RPW);
    head_fwd_rows_kernel<<<d0.N * d0.D * ybl, 256, lds, s>>>(lv, bias, pred, d0.D, d0.H, d0.W);
  } else {
    const long long total4 = (long long)d0.N * d0.vox() / 4;
    head_fwd_kernel<<<grid_for(total4), 256, 0, s>>>(lv, bias, pred, d0.D, d0.H, d0.W, total4);
  }
  SEUNET_LAUNCH_CHECK();
  return 0;
}

// the y- (or z-) passes of all coarse levels of one head in ONE launch: blockIdx.y = job (one per level).  The y launch has
// one more row when the bias gradient is asked for: its first block sums the x pass's bias partials (nothing waits for that
// sum, and it waits for the x pass alone), the others return.
struct AxisJob { const float* in; float* out; int I, O; long long inner, total; };
struct AxisJobs { AxisJob j[3]; int njobs; const double* bias_part; int bias_n; float* g_bias; };
__global__ void __launch_bounds__(256) up_transpose_axis_multi_kernel(AxisJobs jobs) {
  if ((int)blockIdx.y >= jobs.njobs) {
    if (blockIdx.x == 0) sum_stage2_wide_by_256(jobs.bias_part, jobs.bias_n, jobs.g_bias);
    return;
  }
  const AxisJob jb = jobs.j[blockIdx.y];
  if (jb.total == 0) return;
  const float rs = ac_scale(jb.I, jb.O);
  // (32-bit index arithmetic: a 64-bit division costs ~100 vector instructions and this loop has three per output; the launcher
  // checks that every flat index of the job fits)
  const unsigned inner = (unsigned)jb.inner, I = (unsigned)jb.I, total = (unsigned)jb.total;
  for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const unsigned q = idx / inner;
    const unsigned in_i = idx - q * inner;
    const unsigned outer = q / I;
    const int i = (int)(q - outer * I);
    int lo, hi;
    ac_range(i, rs, jb.O, lo, hi);
    float acc = 0.f;
    // four taps at a time: their loads are independent and go out together (same taps, same order of summation)
    for (int o = lo; o <= hi; o += 4) {
      float w[4], v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        w[k] = o + k <= hi ? ac_weight(o + k, i, rs, jb.I) : 0.f;
        v[k] = w[k] != 0.f ? jb.in[(outer * (unsigned)jb.O + (unsigned)(o + k)) * inner + in_i] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (w[k] != 0.f) acc += w[k] * v[k];
    }
    jb.out[idx] = acc;
  }
}

// The workspace of head_bwd, in floats from its start.  head_bwd_tmp_floats() and launch_head_bwd() both take it from
// head_bwd_layout(): x-pass outputs t1[l] = [N][D0][H0][Wl] of the (<= 3) coarse levels (7/8 of a full-resolution map), their
// y-pass outputs t2[l] = [N][D0][Hl][Wl] behind them (<= 21/64), then the bias partials (f64, one per block of the x pass).
struct HeadBwdLayout { long long t1[4], t2[4], part, total; };
static HeadBwdLayout head_bwd_layout(Dims d0, int nlevels) {
  HeadBwdLayout m{};
  const long long rows = (long long)d0.N * d0.D * d0.H, V = rows * d0.W;
  long long off = 0, off2 = V - V / 8;
  for (int l = 1; l < nlevels; ++l) {
    m.t1[l] = off;
    off += rows * (d0.W >> l);
    m.t2[l] = off2;
    off2 += (long long)d0.N * d0.D * (d0.H >> l) * (d0.W >> l);
  }
  m.part = (V + V / 2 + 64 + 1) & ~1ll;
  m.total = V + V / 2 + 64 + 2 * ((rows + HB_ROWS - 1) / HB_ROWS + 64);
  return m;
}
size_t head_bwd_tmp_floats(Dims d0) { return (size_t)head_bwd_layout(d0, 4).total; }
int launch_head_bwd(const float* g_pred, float* const* g_levels, int nlevels, float* tmp, float* g_bias,
                    Dims d0, hipStream_t s) {
  SEUNET_CHECK(nlevels >= 1 && nlevels <= 4, "head: nlevels=%d out of range", nlevels);
  // (a width that 2^(nlevels - 1) does not divide can give an output more than HB_K taps, which the x pass would drop)
  if (int e = head_extents_check("head_bwd", d0, nlevels)) return e;
  const long long rows = (long long)d0.N * d0.D * d0.H;
  const long long V = rows * d0.W;
  const HeadBwdLayout m = head_bwd_layout(d0, nlevels);
  float* t1[4] = {nullptr, nullptr, nullptr, nullptr};      // (a level without a gradient has no x-pass output)
  float* t2[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int l = 1; l < nlevels; ++l) {
    if (g_levels[l]) t1[l] = tmp + m.t1[l];
    t2[l] = tmp + m.t2[l];
  }
  double* part = reinterpret_cast<double*>(tmp + m.part);
  const int nblk = (int)((rows + HB_ROWS - 1) / HB_ROWS);
  SEUNET_CHECK(d0.W <= 1024, "head_bwd: W=%d too large", d0.W);
  SEUNET_CHECK(V / 2 < (1ll << 31), "head_bwd: %lld voxels per call exceed the 32-bit index range of the axis passes", V);
  const size_t lds = ((size_t)4 * (d0.W + HB_PAD) + (size_t)(d0.W - (d0.W >> 3)) * (HB_K + 2)) * sizeof(float);
  head_bwd_x_multi_kernel<<<nblk, 256, lds, s>>>(g_pred, t1[1], t1[2], t1[3], nlevels, d0.W, rows, g_bias ? part : nullptr);
  // y-pass of every level in one launch, then z-pass of every level in one launch
  AxisJobs jy{}, jz{};
  long long max_y = 0, max_z = 0;
  int njobs = 0;
  for (int l = 1; l < nlevels; ++l) {
    if (!g_levels[l]) continue;
    const int Dl = d0.D >> l, Hl = d0.H >> l, Wl = d0.W >> l;
    const long long ty = (long long)d0.N * d0.D * Hl * Wl, tz = (long long)d0.N * Dl * Hl * Wl;
    jy.j[njobs] = AxisJob{t1[l], t2[l], Hl, d0.H, (long long)Wl, ty};
    jz.j[njobs] = AxisJob{t2[l], g_levels[l], Dl, d0.D, (long long)Hl * Wl, tz};
    max_y = ty > max_y ? ty : max_y;
    max_z = tz > max_z ? tz : max_z;
    ++njobs;
  }
  jy.njobs = jz.njobs = njobs;
  if (njobs) {
    if (g_bias) { jy.bias_part = part; jy.bias_n = nblk; jy.g_bias = g_bias; }
    up_transpose_axis_multi_kernel<<<dim3((unsigned)grid_for(max_y), (unsigned)njobs + (g_bias ? 1 : 0)), 256, 0, s>>>(jy);
    up_transpose_axis_multi_kernel<<<dim3((unsigned)grid_for(max_z), (unsigned)njobs), 256, 0, s>>>(jz);
  } else if (g_bias) {   // (no coarse level: the sum is a launch of its own)
    sum_stage2_wide_kernel<<<1, 1024, 0, s>>>(part, nblk, g_bias);
  }
  SEUNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace seunet
