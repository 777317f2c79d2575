// Weight gradient of the 1x1x1 aggregation convolutions (backward of nn.Conv3d(kernel_size=1) at reference SE_UNet.py:42:
// ec63, ec93, dc22, dc42), 16-bit storage:   dW[co][ci] = sum over all voxels v of  X[v][ci] * dY[v][co]
//
// Why a kernel of its own: a 1x1x1 weight gradient has no spatial structure -- it is ONE GEMM with K = all voxels -- and is bound
// by reading X and dY once.  The tiled kernel (wgrad.hip) splits the (ci, co) plane into 32 x 32 combos that each stream their
// own slice of both tensors: for 128 -> 64 channels X is read twice and dY four times, in 64-byte slices of 256-byte voxel
// records (0.169 ms for ec63 against 0.07 ms of HBM time).  Here a workgroup owns ALL (ci, co) pairs and walks chunks of 64 /
// 128 consecutive voxels of the flat [N x D x H x W] index:
//   * the chunk of every source tensor and of dY arrives by LDS-DMA as one contiguous copy (voxel-major records, the 16-byte
//     pieces XOR-swizzled by voxel on the source side so that the transposing reads are conflict-free), two chunks in flight;
//   * the four waves split the 16-channel input blocks, every wave pairs its blocks with all output blocks:
//     v_mfma_f32_16x16x32, A = dY^T (16 channels x 32 voxels), B = X (32 voxels x 16 channels), both through
//     ds_read_b64_tr_b16; accumulators (<= 24 pairs per wave) live in registers for the whole launch;
//   * one slab per workgroup, summed by the family's shared reduction (wgrad.h).
#include "seunet_common.h"
#include "lds_dma.h"
#include "mfma.h"
#include "wgrad.h"
#include <cstdlib>

namespace seunet {

struct W1Args {
  const void* src[3]; int srcC[3]; int nsrc;      // X: up to three tensors of 32 or 64 channels each
  const void* dy; int cout;
  float* slab; const void* zero;
  long long nvox;                                  // N * D * H * W
  int nchunk;
  int nst;                                         // LDS stages (2..4): nst - 1 chunks in flight
};

static constexpr int W1_NW = 4;

// CIBW: 16-channel input blocks per wave; NCOB: 16-channel output blocks (all of them, every wave); CH: voxels per chunk
template <typename T, int CIBW, int NCOB, int CH>
__global__ void __launch_bounds__(256)
wgrad_1x1_kernel(W1Args a) {
  constexpr int KS = CH / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3;
  const int cin = a.srcC[0] + (a.nsrc > 1 ? a.srcC[1] : 0) + (a.nsrc > 2 ? a.srcC[2] : 0);
  const int stage = (cin + a.cout) * 2 * CH;                 // one stage: the X regions of the sources back to back, then dY
  const int dump = a.nst * stage;                            // 1 KB landing area of the padding DMA instructions
  // region offsets of the sources inside a stage
  int roff[3];
  roff[0] = 0; roff[1] = a.srcC[0] * 2 * CH; roff[2] = roff[1] + (a.nsrc > 1 ? a.srcC[1] : 0) * 2 * CH;
  const int yoff0 = cin * 2 * CH;

  // ---- fragment addressing (per lane, chunk-invariant): X block c of this wave / dY block k, K-step ks, half r ----
  unsigned xoff[CIBW][KS][2], yoff[NCOB][KS][2];
#pragma unroll
  for (int c = 0; c < CIBW; ++c) {
    const int ch0 = (wave * CIBW + c) * 16;                  // first channel of the block in the concatenation
    int s = 0, cl = ch0;
    if (a.nsrc > 1 && cl >= a.srcC[0]) { cl -= a.srcC[0]; s = 1; if (a.nsrc > 2 && cl >= a.srcC[1]) { cl -= a.srcC[1]; s = 2; } }
    const int C = a.srcC[s], np = C / 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int v = 32 * ks + 8 * grp + 4 * r + q;
        xoff[c][ks][r] = (unsigned)(roff[s] + v * C * 2 + (((cl / 8 + (p >> 1)) ^ tr16_swz(np, v)) * 16) + (p & 1) * 8);
      }
  }
  {
    const int npy = a.cout / 8;
#pragma unroll
    for (int k = 0; k < NCOB; ++k)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int v = 32 * ks + 8 * grp + 4 * r + q;
          yoff[k][ks][r] = (unsigned)(yoff0 + v * a.cout * 2 + (((k * 2 + (p >> 1)) ^ tr16_swz(npy, v)) * 16) + (p & 1) * 8);
        }
  }

  // ---- DMA plan: instruction number id = wave + 4 * it of a stage image (1 KB each).  Per lane and instruction one packed word:
  //      bits 0-1 tensor (0..2 sources, 3 = dY), bits 4-19 byte offset of the 16-byte piece inside the tensor's chunk (pieces
  //      permuted), bits 20-27 voxel inside the chunk; ~0 = padding.  Every wave issues exactly LW instructions per chunk
  //      (LW = 8, 16 or 24 >= the real count, so that the loop's wait count is one of a few literals; lds_dma.h (a)), the
  //      surplus ones copy the zero page to a dump. ----
  const int ni = stage / 1024;                               // (regions are multiples of 1 KB: channels % 32 == 0, CH >= 64)
  const int items = (ni + W1_NW - 1) / W1_NW;
  const int LW = items <= 8 ? 8 : (items <= 16 ? 16 : 24);   // (uniform)
  constexpr int MAXI = 24;
  unsigned plan[MAXI];
#pragma unroll
  for (int it = 0; it < MAXI; ++it) {
    const int id = wave + W1_NW * it;
    const int byte = id * 1024 + lane * 16;
    int sel, C, rel;
    if (byte >= yoff0) { sel = 3; C = a.cout; rel = byte - yoff0; }
    else if (a.nsrc > 2 && byte >= roff[2]) { sel = 2; C = a.srcC[2]; rel = byte - roff[2]; }
    else if (a.nsrc > 1 && byte >= roff[1]) { sel = 1; C = a.srcC[1]; rel = byte - roff[1]; }
    else { sel = 0; C = a.srcC[0]; rel = byte; }
    const int sh = 31 - __clz(C * 2);                        // records are 64, 128 or 256 bytes
    const int v = rel >> sh, slot = (rel & (C * 2 - 1)) >> 4;
    const int piece = slot ^ tr16_swz(C / 8, v);
    plan[it] = (it < items && id < ni) ? ((unsigned)sel | ((unsigned)((v << sh) + piece * 16) << 4) | ((unsigned)v << 20)) : 0xFFFFFFFFu;
  }
  const unsigned char* zero_page = reinterpret_cast<const unsigned char*>(a.zero) + lane * 16;
  const unsigned char* tb[4] = {reinterpret_cast<const unsigned char*>(a.src[0]), reinterpret_cast<const unsigned char*>(a.nsrc > 1 ? a.src[1] : a.src[0]),
                                reinterpret_cast<const unsigned char*>(a.nsrc > 2 ? a.src[2] : a.src[0]), reinterpret_cast<const unsigned char*>(a.dy)};
  const long long tstride[4] = {(long long)CH * a.srcC[0] * 2, (long long)CH * a.srcC[1] * 2, (long long)CH * a.srcC[2] * 2, (long long)CH * a.cout * 2};
  auto issue = [&](int chunk, int st) __attribute__((always_inline)) {
    const bool cok = chunk < a.nchunk;                       // wave-uniform
    const long long left = a.nvox - (long long)chunk * CH;   // voxels of the volume from this chunk on
    const unsigned char* cb[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) cb[t] = tb[t] + (long long)(cok ? chunk : 0) * tstride[t];
#pragma unroll
    for (int it = 0; it < MAXI; ++it) {
      if (it < LW) {                                         // (uniform)
        const unsigned w = plan[it];
        const int sel = w & 3, v = (w >> 20) & 0xFF;
        const unsigned char* base = sel == 0 ? cb[0] : (sel == 1 ? cb[1] : (sel == 2 ? cb[2] : cb[3]));
        const bool ok = cok && w != 0xFFFFFFFFu && v < left;
        const unsigned char* gp = ok ? base + ((w >> 4) & 0xFFFF) : zero_page;
        const int id = wave + W1_NW * it;
        dma16(gp, (it < items && id < ni) ? lds_base + (unsigned)(st * stage + id * 1024) : lds_base + (unsigned)dump);
      }
    }
  };

  f32x4 acc[CIBW][NCOB];
#pragma unroll
  for (int c = 0; c < CIBW; ++c)
#pragma unroll
    for (int k = 0; k < NCOB; ++k) acc[c][k] = f32x4{0.f, 0.f, 0.f, 0.f};

  // chunks blockIdx.x, blockIdx.x + gridDim.x, ...; PF = nst - 1 chunks are in flight ahead of the one being multiplied (the
  // launch is bound by HBM latency x bytes in flight: two stages of 24 KB per CU were 3.6 TB/s)
  const int nst = a.nst, PF = nst - 1;
  int chunk = blockIdx.x, st = 0, stp = 0;                    // stage of the current chunk / of the next one to issue
  for (int k = 0; k < PF; ++k) { issue(chunk + k * (int)gridDim.x, stp); stp = stp + 1 == nst ? 0 : stp + 1; }
  for (; chunk < a.nchunk; chunk += gridDim.x) {
    issue(chunk + PF * (int)gridDim.x, stp);                 // (beyond the last chunk: padding instructions, same count)
    stp = stp + 1 == nst ? 0 : stp + 1;
    // the current chunk's LW loads are older than the PF * LW issued after them, and no stores are in flight.  wgrad_1x1_cfg
    // gives PF * LW = 8, 16, 24, 32 or 48 (PF = nst - 1 = 1..3, LW = 8 / 16 / 24, product <= 48)
    switch (PF * LW) {
      case 8: wait_loads<8>(); break;
      case 16: wait_loads<16>(); break;
      case 24: wait_loads<24>(); break;
      case 32: wait_loads<32>(); break;
      case 48: wait_loads<48>(); break;
      default: wait_loads<0>(); break;                       // (72: beyond the 6-bit counter; the launcher never asks for it)
    }
    __builtin_amdgcn_s_barrier();
    const unsigned sb = lds_base + (unsigned)(st * stage);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      bf16x8 xf[CIBW], yf[NCOB];
#pragma unroll
      for (int c = 0; c < CIBW; ++c) xf[c] = frag_tr16(sb + xoff[c][ks][0], sb + xoff[c][ks][1]);
#pragma unroll
      for (int k = 0; k < NCOB; ++k) yf[k] = frag_tr16(sb + yoff[k][ks][0], sb + yoff[k][ks][1]);
#pragma unroll
      for (int c = 0; c < CIBW; ++c)
#pragma unroll
        for (int k = 0; k < NCOB; ++k) acc[c][k] = mfma_16x16x32<T>(yf[k], xf[c], acc[c][k]);
    }
    __builtin_amdgcn_s_barrier();                            // every wave is done reading this stage before it is refilled
    st = st + 1 == nst ? 0 : st + 1;
  }
  wait_loads<0>();

  // ---- slab of this workgroup: [wave][c][k][lane][4] ----
  float* out = a.slab + ((size_t)blockIdx.x * W1_NW + wave) * (CIBW * NCOB * 256) + lane * 4;
#pragma unroll
  for (int c = 0; c < CIBW; ++c)
#pragma unroll
    for (int k = 0; k < NCOB; ++k) *reinterpret_cast<f32x4*>(out + (c * NCOB + k) * 256) = acc[c][k];
}

struct W1Cfg { int cibw, ncob, ch, nst; };
static bool wgrad_1x1_cfg(int dtype, const SrcList& x, int cin_logical, int cout, W1Cfg& c) {
  if (dtype_size(dtype) != 2 || x.n < 1 || x.n > 3 || cin_logical != x.total()) return false;
  for (int i = 0; i < x.n; ++i) if (x.C[i] != 32 && x.C[i] != 64) return false;
  if (cout != 32 && cout != 64 && cout != 128) return false;
  const int ncib = cin_logical / 16;
  c.cibw = (ncib + W1_NW - 1) / W1_NW;
  c.ncob = cout / 16;
  if (ncib != W1_NW * c.cibw || c.cibw * c.ncob > 24) return false;
  if (!((c.cibw == 1 && c.ncob == 2) || (c.cibw == 2 && c.ncob == 4) || (c.cibw == 3 && c.ncob == 8))) return false;   // the instantiated forms
  // chunk size and stages: as many bytes in flight as the LDS holds (<= 4 stages; the vmcnt counter is 6 bits: (nst - 1) x
  // padded instructions per chunk <= 48)
  c.ch = 128; c.nst = 0;
  for (int ch = 128; ch >= 64 && c.nst < 3; ch /= 2) {
    const int stage = (cin_logical + cout) * 2 * ch;
    const int items = (stage / 1024 + W1_NW - 1) / W1_NW, lw = items <= 8 ? 8 : (items <= 16 ? 16 : 24);
    if (items > 24) continue;
    int nst = (159 * 1024) / stage;
    if (nst > 4) nst = 4;
    while (nst > 2 && (nst - 1) * lw > 48) --nst;
    if (nst >= 2 && nst > c.nst) { c.nst = nst; c.ch = ch; }
  }
  return c.nst >= 2;
}
bool wgrad_1x1_supported(int dtype, const SrcList& x, int cin_logical, int cout) {
  W1Cfg c;
  return wgrad_1x1_cfg(dtype, x, cin_logical, cout, c);
}

// The launch cut: chunks of the flat voxel index, the persistent workgroups that share them, one slab per workgroup.  A slab is
// [wave][input block of the wave][output block][lane][4]; every admitted configuration has cibw = cin / 64 and ncob = cout / 16,
// and the workspace bound rounds other channel counts up.
static constexpr int W1_MAX_WG = 256;                     // one workgroup per CU
static size_t w1_slab_floats(int cin, int cout) { return (size_t)W1_NW * cdiv(cin, 64) * cdiv(cout, 16) * 256; }
static WgSlabs w1_slabs(int groups, int cin, int cout) { return {WG_SLAB_PREFIX, (size_t)groups, w1_slab_floats(cin, cout)}; }
struct W1Cut { long long nvox; int nchunk, groups; };
static W1Cut w1_cut(const W1Cfg& c, Dims d) {
  W1Cut m;
  m.nvox = (long long)d.N * d.vox();
  m.nchunk = (int)((m.nvox + c.ch - 1) / c.ch);
  m.groups = m.nchunk < W1_MAX_WG ? m.nchunk : W1_MAX_WG;
  return m;
}
size_t wgrad_1x1_workspace_bytes(int cin, int cout) { return w1_slabs(W1_MAX_WG, cin, cout).bytes(); }

template <typename T, int CIBW, int NCOB, int CH>
static int wgrad_1x1_launch(const W1Args& a, int grid, int lds, hipStream_t s) {
  static unsigned long long configured = 0;
  if (int e = configure_kernel_lds(configured, reinterpret_cast<const void*>(&wgrad_1x1_kernel<T, CIBW, NCOB, CH>), lds)) return e;
  wgrad_1x1_kernel<T, CIBW, NCOB, CH><<<grid, 256, lds, s>>>(a);
  SEUNET_LAUNCH_CHECK();
  return 0;
}

int launch_wgrad_1x1(int dtype, const SrcList& x, int cin_logical, const void* dy, int cout, float* dw, void* workspace,
                     size_t ws_bytes, Dims d, hipStream_t s, WgReduceJob* defer) {
  W1Cfg c;
  SEUNET_CHECK(wgrad_1x1_cfg(dtype, x, cin_logical, cout, c),
               "wgrad_1x1: 16-bit tensors, 1..3 sources of 32 or 64 channels (64, 128 or 192 together), 32 / 64 / 128 output channels only");
  const W1Cut cut = w1_cut(c, d);
  const WgSlabs slabs = w1_slabs(cut.groups, cin_logical, cout);
  W1Args a{};
  a.slab = slabs.base(workspace, ws_bytes);
  SEUNET_CHECK(a.slab != nullptr, "wgrad_1x1: workspace too small");
  for (int i = 0; i < 3; ++i) { a.src[i] = i < x.n ? x.ptr[i] : nullptr; a.srcC[i] = i < x.n ? x.C[i] : 0; }
  a.nsrc = x.n;
  a.dy = dy; a.cout = cout;
  a.zero = device_zero_page();
  SEUNET_CHECK(a.zero != nullptr, "wgrad_1x1: cannot allocate the device zero page");
  a.nvox = cut.nvox;
  a.nchunk = cut.nchunk;
  const int grid = cut.groups;
  const int lds = (cin_logical + cout) * 2 * c.ch * c.nst + 1024;
  a.nst = c.nst;
  int e = -1;
  SEUNET_DTYPE_SWITCH(dtype, if constexpr (sizeof(T) == 2) {
    if (c.cibw == 1 && c.ch == 128) e = wgrad_1x1_launch<T, 1, 2, 128>(a, grid, lds, s);
    else if (c.cibw == 1) e = wgrad_1x1_launch<T, 1, 2, 64>(a, grid, lds, s);
    else if (c.cibw == 2 && c.ch == 128) e = wgrad_1x1_launch<T, 2, 4, 128>(a, grid, lds, s);
    else if (c.cibw == 2) e = wgrad_1x1_launch<T, 2, 4, 64>(a, grid, lds, s);
    else if (c.ch == 128) e = wgrad_1x1_launch<T, 3, 8, 128>(a, grid, lds, s);
    else e = wgrad_1x1_launch<T, 3, 8, 64>(a, grid, lds, s);
  });
  if (e) return e;
  return finish_wgrad(a.slab, grid, (int)slabs.per, 1, W1Map{c.cibw, c.ncob, cin_logical}, dw, defer, s);
}

}  // namespace seunet
