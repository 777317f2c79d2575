// Whole-network executor: SE_UNet.forward (reference SE_UNet.py:181-238) and its backward, as one
// stream-ordered sequence of the kernels in this directory.  The graph is data (kOps below) and two small
// interpreters walk it forwards / backwards; nothing here allocates: every intermediate lives at a fixed
// offset of a caller-owned workspace whose layout is a pure function of seunet_net_desc (so the same
// layout is recomputed by the backward call).
#include "seunet_common.h"
#include "epilogue.h"
#include "wgrad.h"
#include "../../include/seunet_hip.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace seunet {

// kernel routing, the part other files call (wgrad.h): the non-streaming weight gradient's kernel by size.  The rest of the
// routing is Plan::route below.
ConvKernel wgrad_kernel(int dtype, int taps, int dil, const SrcList& x, int cin_logical, int cout, Dims d, long long src_dist) {
  if (taps == 1) {
    // where the whole-GEMM 1x1x1 kernel beats the tiled kernel (isolated launches): many (ci, co) combos there, i.e. many
    // re-reads -- ec63 (8 combos, 1 M voxels) 0.104 vs 0.165 ms, 192 -> 128 channels (24 combos, 131 k voxels) 0.051 vs 0.085 ms;
    // not dc42 (2 combos: 0.059 vs 0.039 ms) nor dc22 (8 combos but 131 k voxels: 0.033 vs 0.023 ms, four chunks per workgroup do
    // not amortise the pipeline fill).  (ec93 is 192 -> 64 at width 1: 12 combos on 131 k voxels, on dc22's side, and not a form
    // wgrad_1x1.hip instantiates.)
    const int combos = cdiv(cin_logical, 32) * cdiv(cout, 32);
    const long long nv = (long long)d.N * d.vox();
    const bool pays = combos >= 16 || (combos >= 8 && nv >= 500000);
    return pays && wgrad_1x1_supported(dtype, x, cin_logical, cout) ? ConvKernel::Wgrad1x1 : ConvKernel::Tiled;
  }
  // where the marching kernel beats the tiled kernel (isolated launches, 4 samples): the fine levels (rows of >= 32 voxels,
  // >= 48^3); every dilation-2 layer down to 16^3 (the tiled kernel works on parity sub-lattices there: 32^3 64 -> 64 0.057 vs
  // 0.080 ms, 16^3 128 -> 128 0.058 vs 0.075 ms); 256-channel inputs (dc1 at width 2: 0.118 vs 0.134 ms; 128 at width 1).  Dilation 1 with <= 128 input
  // channels on the coarse levels is a tie and stays where it was.
  const bool fine = d.W >= 32 && (long long)d.D * d.H * d.W >= 48LL * 48 * 48;
  const bool pays = fine || dil == 2 || cin_logical >= 256;
  return pays && wgrad_march_supported(dtype, taps, dil, x, cin_logical, cout, d, src_dist) ? ConvKernel::March : ConvKernel::Tiled;
}

namespace {

// ---------------------------------------------------------------------------------------------------
// parameter registry == the reference's state_dict order (SE_UNet.py:108-151)
// ---------------------------------------------------------------------------------------------------
struct BlockDesc { const char* name; char kind; int cin; int cout; };  // cin -1 = in_channel; 'g' one gate, 'G' two, 'c' cat
const BlockDesc kBlocks[] = {
    {"ec1", 'g', -1, 8},   {"ec2", 'g', 8, 16},    {"ec3", 'g', 16, 32},  {"ec33", 'c', 56, 32},  {"x33", 'c', -1, 32},
    {"ec4", 'G', 32, 32},  {"ec5", 'G', 32, 32},   {"ec6", 'G', 32, 64},  {"ec63", 'c', 128, 64}, {"x63", 'c', -1, 64},
    {"ec7", 'G', 64, 64},  {"ec8", 'G', 64, 64},   {"ec9", 'G', 64, 64},  {"ec93", 'c', 192, 64}, {"x93", 'c', -1, 64},
    {"ec10", 'G', 64, 64}, {"ec11", 'G', 64, 64},  {"ec12", 'G', 64, 64}, {"ec123", 'c', 192, 64},
    {"dc1", 'G', 128, 64}, {"dc2", 'G', 64, 64},   {"dc22", 'c', 128, 64},
    {"dc3", 'G', 128, 64}, {"dc4", 'G', 64, 32},   {"dc42", 'c', 96, 32},
    {"dc5", 'g', 64, 32},  {"dc6", 'g', 32, 16},   {"dc62", 'c', 48, 16},
};
constexpr int kNumBlocks = sizeof(kBlocks) / sizeof(kBlocks[0]);

struct ParamInfo { std::string name; int shape[5]; int ndim; };
// registry indices of a block's parameters, -1 = none; xw: for an op, the weight of its aggregation block's x-branch (x33 / x63 / x93)
struct BlockParams { int conv1_w = -1, conv1_b = -1, conv2_w = -1, conv2_b = -1, se = -1, se2 = -1, xw = -1; };

// blocks / head_w / head_b (optional): where the parameters of kBlocks[i] and of the two heads (dc0_0, dc0_1) are in the registry
std::vector<ParamInfo> build_registry(const seunet_net_desc& d, BlockParams* blocks = nullptr, int* head_w = nullptr,
                                      int* head_b = nullptr) {
  std::vector<ParamInfo> r;
  auto add5 = [&](const std::string& n, int a, int b, int k) { r.push_back({n, {a, b, k, k, k}, 5}); return (int)r.size() - 1; };
  auto add1 = [&](const std::string& n, int a) { r.push_back({n, {a, 0, 0, 0, 0}, 1}); return (int)r.size() - 1; };
  for (int i = 0; i < kNumBlocks; ++i) {
    const BlockDesc& b = kBlocks[i];
    const int ci = b.cin < 0 ? d.in_channel : b.cin * d.width_mult, co = b.cout * d.width_mult;
    const std::string n = b.name;
    BlockParams bp;
    bp.conv1_w = add5(n + ".conv1.weight", co, ci, b.kind == 'c' ? 1 : 3);
    if (b.kind != 'c') {
      bp.conv1_b = add1(n + ".conv1.bias", co);
      bp.conv2_w = add5(n + ".conv2.weight", 2, co, 1);
      bp.conv2_b = add1(n + ".conv2.bias", 2);
      bp.se = add5(n + ".conv_se.weight", 1, co, 1);
      if (b.kind == 'G') bp.se2 = add5(n + ".conv_se2.weight", 1, co, 1);
    }
    if (blocks) blocks[i] = bp;
  }
  const int hw0 = add5("dc0_0.weight", d.n_classes, 24, 1), hb0 = add1("dc0_0.bias", d.n_classes);
  const int hw1 = add5("dc0_1.weight", d.n_classes, 12, 1), hb1 = add1("dc0_1.bias", d.n_classes);
  if (head_w) { head_w[0] = hw0; head_w[1] = hw1; }
  if (head_b) { head_b[0] = hb0; head_b[1] = hb1; }
  return r;
}

int find_block(const char* name) {
  for (int i = 0; i < kNumBlocks; ++i)
    if (strcmp(kBlocks[i].name, name) == 0) return i;
  return -1;
}

// ---------------------------------------------------------------------------------------------------
// the graph
// ---------------------------------------------------------------------------------------------------
enum TId {
  T_X0, T_X1, T_X2,
  T_E0, T_E1A, T_E1_1, T_E1, T_E2IN, T_E2, T_E3A, T_E3_1, T_E3, T_E4IN, T_E4, T_E5A, T_E5_1, T_E5,
  T_E6IN, T_E6, T_E7A, T_E7_1, T_E7, T_E8, T_D0A, T_D0_1, T_D0, T_D1U, T_D1A, T_D1_1, T_D1, T_D2U, T_D2A, T_D2_1,
  T_COUNT
};
struct TDesc { int level; int cbase; };  // cbase 0 = padded network input (8 channels)
const TDesc kT[T_COUNT] = {
    {0, 0}, {1, 0}, {2, 0},
    {0, 8}, {0, 16}, {0, 32}, {0, 32}, {1, 32}, {1, 32}, {1, 32}, {1, 64}, {1, 64}, {2, 64}, {2, 64}, {2, 64}, {2, 64}, {2, 64},
    {3, 64}, {3, 64}, {3, 64}, {3, 64}, {3, 64}, {2, 64}, {2, 64}, {2, 64}, {2, 64}, {1, 64}, {1, 64}, {1, 32}, {1, 32}, {0, 32}, {0, 32}, {0, 16},
};

enum OpKind { OP_GATED, OP_CAT, OP_POOL, OP_UP };
struct OpDesc {
  OpKind kind; const char* name; int nsrc; int src[3]; int dst;
  int dil; int gates; int head; int m;   // gated: dilation, #gates, 0 = encoder head / 1 = decoder head, side slot
  const char* xname; int xsrc;          // cat: optional raw-input branch
};
const OpDesc kOps[] = {
    {OP_GATED, "ec1", 1, {T_X0, 0, 0}, T_E0, 1, 1, 0, 0, nullptr, 0},
    {OP_GATED, "ec2", 1, {T_E0, 0, 0}, T_E1A, 1, 1, 0, 1, nullptr, 0},
    {OP_GATED, "ec3", 1, {T_E1A, 0, 0}, T_E1_1, 2, 1, 0, 2, nullptr, 0},
    {OP_CAT, "ec33", 3, {T_E1_1, T_E0, T_E1A}, T_E1, 0, 0, 0, 0, "x33", T_X0},
    {OP_POOL, "pool0", 1, {T_E1, 0, 0}, T_E2IN, 0, 0, 0, 0, nullptr, 0},
    {OP_POOL, "pool0x", 1, {T_X0, 0, 0}, T_X1, 0, 0, 0, 0, nullptr, 0},
    {OP_GATED, "ec4", 1, {T_E2IN, 0, 0}, T_E2, 1, 2, 0, 3, nullptr, 0},
    {OP_GATED, "ec5", 1, {T_E2, 0, 0}, T_E3A, 2, 2, 0, 4, nullptr, 0},
    {OP_GATED, "ec6", 1, {T_E3A, 0, 0}, T_E3_1, 2, 2, 0, 5, nullptr, 0},
    {OP_CAT, "ec63", 3, {T_E3_1, T_E2, T_E3A}, T_E3, 0, 0, 0, 0, "x63", T_X1},
    {OP_POOL, "pool1", 1, {T_E3, 0, 0}, T_E4IN, 0, 0, 0, 0, nullptr, 0},
    {OP_POOL, "pool1x", 1, {T_X1, 0, 0}, T_X2, 0, 0, 0, 0, nullptr, 0},
    {OP_GATED, "ec7", 1, {T_E4IN, 0, 0}, T_E4, 1, 2, 0, 6, nullptr, 0},
    {OP_GATED, "ec8", 1, {T_E4, 0, 0}, T_E5A, 2, 2, 0, 7, nullptr, 0},
    {OP_GATED, "ec9", 1, {T_E5A, 0, 0}, T_E5_1, 2, 2, 0, 8, nullptr, 0},
    {OP_CAT, "ec93", 3, {T_E5_1, T_E4, T_E5A}, T_E5, 0, 0, 0, 0, "x93", T_X2},
    {OP_POOL, "pool2", 1, {T_E5, 0, 0}, T_E6IN, 0, 0, 0, 0, nullptr, 0},
    {OP_GATED, "ec10", 1, {T_E6IN, 0, 0}, T_E6, 1, 2, 0, 9, nullptr, 0},
    {OP_GATED, "ec11", 1, {T_E6, 0, 0}, T_E7A, 1, 2, 0, 10, nullptr, 0},
    {OP_GATED, "ec12", 1, {T_E7A, 0, 0}, T_E7_1, 1, 2, 0, 11, nullptr, 0},
    {OP_CAT, "ec123", 3, {T_E7_1, T_E6, T_E7A}, T_E7, 0, 0, 0, 0, nullptr, 0},
    {OP_UP, "up0", 1, {T_E7, 0, 0}, T_E8, 0, 0, 0, 0, nullptr, 0},
    {OP_GATED, "dc1", 2, {T_E8, T_E5, 0}, T_D0A, 1, 2, 1, 0, nullptr, 0},
    {OP_GATED, "dc2", 1, {T_D0A, 0, 0}, T_D0_1, 1, 2, 1, 1, nullptr, 0},
    {OP_CAT, "dc22", 2, {T_D0_1, T_D0A, 0}, T_D0, 0, 0, 0, 0, nullptr, 0},
    {OP_UP, "up1", 1, {T_D0, 0, 0}, T_D1U, 0, 0, 0, 0, nullptr, 0},
    {OP_GATED, "dc3", 2, {T_D1U, T_E3, 0}, T_D1A, 1, 2, 1, 2, nullptr, 0},
    {OP_GATED, "dc4", 1, {T_D1A, 0, 0}, T_D1_1, 1, 2, 1, 3, nullptr, 0},
    {OP_CAT, "dc42", 2, {T_D1_1, T_D1A, 0}, T_D1, 0, 0, 0, 0, nullptr, 0},
    {OP_UP, "up2", 1, {T_D1, 0, 0}, T_D2U, 0, 0, 0, 0, nullptr, 0},
    {OP_GATED, "dc5", 2, {T_D2U, T_E1, 0}, T_D2A, 1, 1, 1, 4, nullptr, 0},
    {OP_GATED, "dc6", 1, {T_D2A, 0, 0}, T_D2_1, 1, 1, 1, 5, nullptr, 0},
    // dc62 (SE_UNet.py:148,230) is dead: never evaluated, no gradient
};
constexpr int kNumOps = sizeof(kOps) / sizeof(kOps[0]);

inline bool is_input(int t) { return t <= T_X2; }

// ---------------------------------------------------------------------------------------------------
// kernel routing: which kernel runs each pass of each conv (Plan::route, and wgrad_kernel above for the non-streaming weight
// gradient).  The packed weights, the statistics slots, the workspace and the dispatch all follow from that one choice.
// ---------------------------------------------------------------------------------------------------
// levels on which the marching conv pays: full 32-voxel rows and enough (y, x) patches x planes for one workgroup per CU
// (dilation 2 already at 32^3: the tiled kernel runs it on eight 16^3 parity sub-lattices, where its tiles are mostly halo --
// measured on 4 x 32^3, 64 -> 64 channels: forward 0.043 vs 0.057 ms, data gradient 0.039 vs 0.059 ms; dilation 1 at that size
// stays on the tiled kernel, 0.036 vs 0.041 ms)
inline bool march_level(const Dims& d, int dil) {
  return d.W >= 32 && (d.vox() >= 48LL * 48 * 48 || (dil == 2 && d.vox() >= 32LL * 32 * 32));
}

// statistics slots per sample of a forward conv on kernel k
int conv_slots(ConvKernel k, const Dims& dm, int taps, int dil, int cin, int cout) {
  switch (k) {
    case ConvKernel::Stream: return conv_stream_slots(dm, dil);
    case ConvKernel::March: return conv_march_slots(dm, dil, cin, cout);
    case ConvKernel::Naive: return epi_partials(dm);
    default: return conv_stats_tiles(dm, taps, dil);
  }
}

// ---------------------------------------------------------------------------------------------------
// workspace plan
// ---------------------------------------------------------------------------------------------------
struct OpRes {
  size_t raw = 0, raw2 = 0, mean = 0, rstd = 0, mean2 = 0, rstd2 = 0, xtot = 0, wp_f = 0, wp_d = 0, wp_x = 0;
  int cin = 0, cout = 0, taps = 0;
  bool need_dgrad = false;
  // the kernel of each pass (Plan::route): the block conv's forward / data gradient / weight gradient, and the forward / weight
  // gradient of a materialised x-branch (in_channel > 2)
  ConvKernel fwd = ConvKernel::Tiled, dgrad = ConvKernel::Tiled, wgrad = ConvKernel::Tiled;
  ConvKernel x_fwd = ConvKernel::Tiled, x_wgrad = ConvKernel::Tiled;
  size_t pool_idx = 0; bool has_pool_idx = false;              // OP_POOL behind a fused aggregation block: arg-max words of the forward
  size_t side = 0;                                             // n_classes > 1: the block's 2-channel side map, f32 [N][V][2] (classes.hip)
};

struct Plan {
  seunet_net_desc d;
  size_t esz;
  Dims dims[4];
  int C[T_COUNT];
  size_t feat[T_COUNT], grad[T_COUNT];
  OpRes op[kNumOps];
  size_t lvl[2][4], glvl[2][4];
  size_t stats, stats2, pgrad, m1, m2, m1b, m2b, wgrad_ws, head_tmp, gx, gx_bytes = 0, xwp = 0, xmom = 0;
  size_t gside = 0, cls_part = 0, cls_bias = 0;                // n_classes > 1: side-map gradient of one block, head-gradient records, per-(sample, class) bias sums
  // x-branches (x33 / x63 / x93) recomputed from the <= 2-channel input instead of materialised (csrc/cat.hip, XR)
  bool fuse_x = false;
  size_t wgrad_ws_bytes;
  size_t total;
  int stat_slots_max;
  // input gradient (seunet_net_backward_input): a SEPARATE caller-owned scratch buffer, laid out here so that the workspace (and
  // seunet_net_workspace_bytes) stays what it is -- the per-level x-branch terms gx_l = W_xl^T d2_xl, f32 [N][V_l][in_channel]
  size_t ig_gx[3] = {0, 0, 0}, ig_total = 0;
  void plan_input_grad() {
    size_t c = 0;
    for (int l = 0; l < 3; ++l) { ig_gx[l] = c; c = align_up(c + (size_t)d.batch * dims[l].vox() * d.in_channel * 4, 256); }
    ig_total = c;
  }

  size_t cur = 0;
  size_t take(size_t bytes) { size_t o = cur; cur = align_up(cur + bytes, 256); return o; }

  // The kernel of every conv pass of op i (OpRes::fwd .. x_wgrad).
  void route(int i) {
    const OpDesc& o = kOps[i];
    OpRes& r = op[i];
    if (d.conv_impl == SEUNET_CONV_NAIVE) { r.fwd = r.dgrad = r.wgrad = r.x_fwd = r.x_wgrad = ConvKernel::Naive; return; }
    const Dims& dm = dims[kT[o.dst].level];
    SrcList x{}, gy{};   // the forward's sources and the data gradient's
    DstList y{}, gx{};   // and their destinations
    x.n = gx.n = o.nsrc;
    for (int k = 0; k < o.nsrc; ++k) x.C[k] = gx.C[k] = C[o.src[k]];
    y.n = gy.n = 1;
    y.C[0] = gy.C[0] = r.cout;
    const int c0 = C[o.src[0]];
    // small-channel 3x3x3 layers with one source tensor (ec1 / ec2 / ec3 / dc6 at width 1) run on the streaming kernel
    // (the streaming kernels address one sample through 32-bit buffer offsets; a sample of 4 GB or more takes the general kernels)
    const bool stream_ok = o.kind == OP_GATED && o.nsrc == 1 && (long long)dm.D * dm.H * dm.W * 32 * (long long)esz < 0xFFFFFFFFll;
    const bool stream_f = stream_ok && conv_stream_supported(d.dtype, 27, o.dil, c0, r.cout);
    const bool stream_d = stream_ok && conv_stream_supported(d.dtype, 27, o.dil, r.cout, c0);
    // 32 / 64-input-channel 3x3x3 layers of the levels that fill the chip with 32-voxel rows run on the marching kernel
    // (one workgroup per CU, weights in registers): dc5, dc4, ec4..ec6 and the data gradients of those and of dc3
    const bool march_ok = o.kind == OP_GATED && !stream_f && march_level(dm, o.dil);
    r.fwd = stream_f ? ConvKernel::Stream
          : march_ok && conv_march_supported(d.dtype, 27, o.dil, x, y) ? ConvKernel::March : ConvKernel::Tiled;
    r.dgrad = stream_d ? ConvKernel::Stream
            : march_ok && conv_march_supported(d.dtype, 27, o.dil, gy, gx) ? ConvKernel::March : ConvKernel::Tiled;
    // (the marching weight gradient reaches both sources of dc5 through one 32-bit descriptor: their distance counts)
    const long long src_dist = o.nsrc == 2 ? (long long)feat[o.src[1]] - (long long)feat[o.src[0]] : 0;
    r.wgrad = stream_ok && wgrad_stream_supported(d.dtype, 27, o.dil, c0, r.cout)
                  ? ConvKernel::Stream : wgrad_kernel(d.dtype, r.taps, o.dil, x, r.cin, r.cout, dm, src_dist);
    if (o.xname) {   // the x-branch: 1x1x1 conv of the 8-channel padded input
      SrcList xs{};
      xs.n = 1; xs.C[0] = 8;
      r.x_fwd = ConvKernel::Tiled;
      r.x_wgrad = wgrad_kernel(d.dtype, 1, 1, xs, d.in_channel, r.cout, dm, 0);
    }
  }
  // bytes of a packed weight for kernel k: src_c channels in the single source tensor (Stream), cin -> cout channels
  size_t wpack_bytes(ConvKernel k, int taps, int src_c, int cin, int cout) const {
    switch (k) {
      case ConvKernel::Stream: return conv_stream_wpack_bytes(src_c);
      case ConvKernel::March: return conv_march_wpack_bytes(cin, cout);
      default: return conv_wpack_bytes(d.dtype, taps, cin, cout);   // (the naive kernels read the PyTorch weight: same slot)
    }
  }

  int init(const seunet_net_desc& desc) {
    d = desc;
    SEUNET_CHECK(d.batch >= 1 && d.in_channel >= 1 && d.in_channel <= 8, "net: batch/in_channel out of range");
    SEUNET_CHECK(d.n_classes >= 1 && d.n_classes <= class_max(), "net: n_classes=%d out of range (1 .. %d)", d.n_classes, class_max());
    SEUNET_CHECK(d.d % 8 == 0 && d.h % 8 == 0 && d.w % 8 == 0 && d.d >= 8 && d.h >= 8 && d.w >= 8,
                 "net: spatial extents (%d,%d,%d) must be multiples of 8", d.d, d.h, d.w);
    SEUNET_CHECK(d.width_mult == 1 || d.width_mult == 2, "net: width_mult %d unsupported (1 or 2)", d.width_mult);
    SEUNET_CHECK(dtype_ok(d.dtype), "net: dtype %d unsupported (SEUNET_F32 | SEUNET_BF16 | SEUNET_F16)", d.dtype);
    esz = dtype_size(d.dtype);
    for (int l = 0; l < 4; ++l) dims[l] = Dims{d.batch, d.d >> l, d.h >> l, d.w >> l};
    for (int t = 0; t < T_COUNT; ++t) C[t] = kT[t].cbase == 0 ? 8 : kT[t].cbase * d.width_mult;
    // (the two sources of a two-source marching layer are allocated next to each other: the kernel then reaches both through one
    // 32-bit buffer descriptor, conv_march.hip `BUF` and wgrad_march.hip)
    bool placed[T_COUNT] = {};
    for (int t = 0; t < T_COUNT; ++t) {
      const size_t bytes = (size_t)d.batch * dims[kT[t].level].vox() * C[t] * esz;
      if (!placed[t]) { feat[t] = take(bytes); placed[t] = true; }
      // (dc5 only.  The same placement for dc3 and dc1 cost their tiled forward 5 % -- conv_fwd:dc3 0.465 -> 0.49 ms, same box,
      // alternating runs -- and their sources are 1.2 GB apart at batch 4 anyway; beyond 4 GB the weight gradient of those two
      // layers takes the tiled kernel)
      const int mate = t == T_E1 ? T_D2U : -1;
      if (mate >= 0 && !placed[mate]) {
        feat[mate] = take((size_t)d.batch * dims[kT[mate].level].vox() * C[mate] * esz);
        placed[mate] = true;
      }
      grad[t] = is_input(t) ? 0 : take(bytes);
    }
    size_t gx_max = 0, wg_max = 0, xw_max = 0, xmom_max = 0;
    fuse_x = d.in_channel <= 2 && d.conv_impl != SEUNET_CONV_NAIVE;
    int slots_max = 1, cmax = 8;
    for (int i = 0; i < kNumOps; ++i) {
      const OpDesc& o = kOps[i];
      OpRes& r = op[i];
      if (o.kind == OP_POOL && i > 0 && kOps[i - 1].kind == OP_CAT && kOps[i - 1].xname && kOps[i - 1].dst == o.src[0] &&
          fuse_x && !is_input(o.src[0])) {
        // the aggregation block's forward writes this pool (and the position of each maximum, which the backward pass then
        // reads instead of the block output and the pooled tensor)
        const Dims& dl = dims[kT[o.dst].level];
        r.pool_idx = take((size_t)d.batch * dl.vox() * (C[o.src[0]] / 8) * 4);
        r.has_pool_idx = true;
      }
      if (o.kind == OP_POOL || o.kind == OP_UP) continue;
      const int lv = kT[o.dst].level;
      r.cout = C[o.dst];
      r.taps = o.kind == OP_GATED ? 27 : 1;
      int cin = 0;
      bool any_grad = false;
      for (int k = 0; k < o.nsrc; ++k) { cin += C[o.src[k]]; any_grad |= !is_input(o.src[k]); }
      if (o.nsrc == 1 && is_input(o.src[0])) cin = d.in_channel;
      r.cin = cin;
      r.need_dgrad = any_grad;
      const size_t act = (size_t)d.batch * dims[lv].vox() * r.cout * esz;
      r.raw = take(act);
      r.mean = take((size_t)d.batch * r.cout * 4);
      r.rstd = take((size_t)d.batch * r.cout * 4);
      route(i);
      r.wp_f = take(wpack_bytes(r.fwd, r.taps, C[o.src[0]], r.cin, r.cout));
      if (r.need_dgrad) r.wp_d = take(wpack_bytes(r.dgrad, r.taps, r.cout, r.cout, r.cin));
      slots_max = std::max(slots_max, conv_slots(r.fwd, dims[lv], r.taps, o.dil, cin, r.cout));
      if (r.wgrad == ConvKernel::Stream) wg_max = std::max(wg_max, wgrad_stream_workspace_bytes(C[o.src[0]], r.cout, o.dil, dims[lv]));
      wg_max = std::max(wg_max, wgrad_workspace_bytes(r.taps, r.cin, r.cout));
      if (o.xname) {
        r.mean2 = take((size_t)d.batch * r.cout * 4);
        r.rstd2 = take((size_t)d.batch * r.cout * 4);
        if (fuse_x) {
          xw_max = std::max(xw_max, (size_t)d.batch * epi_partials(dims[lv]) * r.cout * 2 * 8);
          r.xtot = take((size_t)d.batch * 5 * 8);      // the input's moments per sample, kept for the backward pass
          xmom_max = std::max(xmom_max, (size_t)d.batch * xbranch_moment_slots(dims[lv]) * 5 * 8);
        } else {
          r.raw2 = take(act);
          r.wp_x = take(wpack_bytes(r.x_fwd, 1, 8, d.in_channel, r.cout));
          gx_max = std::max(gx_max, act);
          wg_max = std::max(wg_max, wgrad_workspace_bytes(1, d.in_channel, r.cout));
        }
      }
      slots_max = std::max(slots_max, std::max(std::max(conv_stats_tiles(dims[lv], 27, 1), conv_stats_tiles(dims[lv], 27, 2)), epi_partials(dims[lv])));
      cmax = std::max(cmax, r.cout);
      if (d.n_classes > 1 && o.kind == OP_GATED) r.side = take((size_t)d.batch * dims[lv].vox() * 2 * 4);
    }
    stat_slots_max = slots_max;
    for (int h = 0; h < 2; ++h)
      for (int l = 0; l < 4; ++l) {
        lvl[h][l] = take((size_t)d.n_classes * d.batch * dims[l].vox() * 4);       // [class][N][V]
        glvl[h][l] = take((size_t)d.n_classes * d.batch * dims[l].vox() * 4);
      }
    if (d.n_classes > 1) {
      gside = take((size_t)d.batch * dims[0].vox() * 2 * 4);
      cls_part = take((size_t)d.batch * 256 * 2 * d.n_classes * 8);
      cls_bias = take((size_t)d.batch * d.n_classes * 4);
    }
    const size_t stat_bytes = (size_t)d.batch * slots_max * cmax * 2 * 8;   // f32 forward / f64 backward partials
    stats = take(stat_bytes);
    stats2 = take(stat_bytes);
    pgrad = take((size_t)d.batch * slots_max * (4 * cmax + 4) * 4);
    m1 = take((size_t)d.batch * cmax * 4);
    m2 = take((size_t)d.batch * cmax * 4);
    m1b = take((size_t)d.batch * cmax * 4);
    m2b = take((size_t)d.batch * cmax * 4);
    wgrad_ws_bytes = wg_max;
    wgrad_ws = take(wg_max);
    head_tmp = take(head_bwd_tmp_floats(dims[0]) * 4);
    gx = take(gx_max);
    gx_bytes = gx_max;
    xwp = take(xw_max);
    xmom = take(xmom_max);
    total = cur;
    plan_input_grad();
    return 0;
  }
};

struct Exec {
  Plan p;
  unsigned char* ws = nullptr;
  const float* const* params = nullptr;
  hipStream_t s = nullptr;
  float* grad_x = nullptr;             // seunet_net_backward_input: NCDHW f32 input gradient (null = not requested)
  unsigned char* igs = nullptr;        // its scratch buffer (Plan::ig_gx)

  BlockParams opp[kNumOps];            // parameter indices of each op's block and of the two heads, resolved once in setup
  int head_w[2], head_b[2];
  const float* drops[2] = {nullptr, nullptr};   // DropLayer scales of the encoder / decoder head, or null

  float* gxl(int l) const { return reinterpret_cast<float*>(igs + p.ig_gx[l]); }
  void mark(const char* tag, const char* name = "") const { if (prof_on()) prof_mark((std::string(tag) + name).c_str(), s); }
  void* at(size_t off) const { return ws + off; }
  float* fat(size_t off) const { return reinterpret_cast<float*>(ws + off); }
  double* dat(size_t off) const { return reinterpret_cast<double*>(ws + off); }
  const float* par(int i) const { return i < 0 ? nullptr : params[i]; }

  int setup(const seunet_net_desc* desc, const float* const* prm, void* workspace, size_t bytes, hipStream_t st) {
    SEUNET_CHECK(desc && prm && workspace, "net: null argument");
    if (int e = p.init(*desc)) return e;
    SEUNET_CHECK(bytes >= p.total, "net: workspace too small (%zu < %zu bytes)", bytes, p.total);
    SEUNET_CHECK((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "net: workspace must be 256-byte aligned");
    BlockParams blocks[kNumBlocks];
    const std::vector<ParamInfo> reg = build_registry(p.d, blocks, head_w, head_b);
    for (int i = 0; i < kNumOps; ++i) {
      const OpDesc& o = kOps[i];
      if (o.kind != OP_GATED && o.kind != OP_CAT) continue;
      const int b = find_block(o.name), bx = o.xname ? find_block(o.xname) : -1;
      SEUNET_CHECK(b >= 0 && (!o.xname || bx >= 0), "net: internal: no parameters for %s", o.name);
      opp[i] = blocks[b];
      if (bx >= 0) opp[i].xw = blocks[bx].conv1_w;
    }
    ws = reinterpret_cast<unsigned char*>(workspace);
    params = prm;
    s = st;
    for (size_t i = 0; i < reg.size(); ++i)
      SEUNET_CHECK(prm[i] != nullptr || reg[i].name.rfind("dc62", 0) == 0, "net: parameter %s is null", reg[i].name.c_str());
    return 0;
  }

  SrcList srcs(const OpDesc& o) const {
    SrcList l{};
    l.n = o.nsrc;
    for (int k = 0; k < o.nsrc; ++k) { l.ptr[k] = at(p.feat[o.src[k]]); l.C[k] = p.C[o.src[k]]; }
    return l;
  }

  // one forward or data-gradient conv on kernel k.  w: the PyTorch weight (naive kernels, tflip 1 = data gradient); wp: the weight
  // packed for k by pack_all_weights
  int run_conv(ConvKernel k, int taps, int dil, const SrcList& src, int cin, const float* w, int tflip, const void* wp,
               const float* bias, const DstList& dst, double* stats, const Dims& dm) const {
    switch (k) {
      case ConvKernel::Naive: return launch_conv_naive(p.d.dtype, taps, dil, src, cin, w, tflip, bias, dst, dm, s);
      case ConvKernel::Tiled: return launch_conv_igemm(p.d.dtype, taps, dil, src, cin, wp, bias, dst, stats, dm, s);
      case ConvKernel::Stream:
        return launch_conv_stream(p.d.dtype, dil, src.ptr[0], src.C[0], wp, bias, dst.ptr[0], dst.C[0], dst.acc[0], stats, dm, s);
      case ConvKernel::March: return launch_conv_march(p.d.dtype, dil, src, wp, bias, dst, stats, dm, s);
      default: return fail("net: internal: kernel %d runs no convolution", (int)k);
    }
  }

  // conv (+ InstanceNorm statistics) of one block: raw <- conv(src), (mean, rstd) <- stats(raw)
  int conv_and_stats(const char* nm, ConvKernel k, int taps, int dil, const SrcList& src, int cin, const float* w,
                     const float* bias, size_t wp_off, size_t raw_off, int cout, size_t mean_off, size_t rstd_off, const Dims& dm) {
    DstList dst{};
    dst.n = 1; dst.ptr[0] = at(raw_off); dst.C[0] = cout; dst.acc[0] = 0;
    mark("conv_fwd:", nm);
    if (int e = run_conv(k, taps, dil, src, cin, w, 0, at(wp_off), bias, dst, dat(p.stats), dm)) return e;
    if (k == ConvKernel::Naive) {   // (the naive conv leaves the statistics to a pass of their own)
      mark("stats");
      if (int e = launch_channel_stats(p.d.dtype, at(raw_off), cout, dat(p.stats), dm, s)) return e;
    }
    mark("stats");
    return launch_stats_finalize(dat(p.stats), conv_slots(k, dm, taps, dil, src.total(), cout), cout, dm.N, dm.vox(), p.d.eps, 0,
                                 fat(mean_off), fat(rstd_off), s);
  }

  // a block's epilogue, described once from its OpRes offsets for the forward and both backward passes
  GateBlock gate_block(int i) const {
    const OpRes& r = p.op[i];
    const BlockParams& bp = opp[i];
    return GateBlock{{at(r.raw), fat(r.mean), fat(r.rstd)}, r.cout,
                     {par(bp.se), par(bp.se2), par(bp.conv2_w), par(bp.conv2_b), p.d.negative_slope}};
  }
  CatBlock cat_block(int i) const {
    const OpDesc& o = kOps[i];
    const OpRes& r = p.op[i];
    Branch2 x{};
    if (o.xname && p.fuse_x) x = {Branch2::Recomputed, at(p.feat[o.xsrc]), fat(r.mean2), fat(r.rstd2), par(opp[i].xw), p.d.in_channel};
    else if (o.xname) x = {Branch2::Stored, at(r.raw2), fat(r.mean2), fat(r.rstd2), nullptr, 0};
    return CatBlock{{at(r.raw), fat(r.mean), fat(r.rstd)}, x, r.cout, p.d.negative_slope};
  }
  // the source of a materialised x-branch conv: the padded network input
  SrcList xbranch_src(const OpDesc& o) const { return SrcList{{at(p.feat[o.xsrc])}, {8}, 1}; }
  bool skip_enc_head = false;   // inference (prediction.py:102-103 discards pred0): the encoder head and its side maps are not evaluated

  // the slice of its head (dc0_0: 24 side channels, dc0_1: 12) that a gated block's two side channels feed
  struct HeadSlice { const float* w; const float* drop; int stride; float* gw; };
  HeadSlice head_slice(const OpDesc& o, float* const* grads = nullptr) const {
    const float* dr = drops[o.head];
    float* g = grads ? grads[head_w[o.head]] : nullptr;
    return HeadSlice{params[head_w[o.head]] + 2 * o.m, dr ? dr + 2 * o.m : nullptr, o.head == 0 ? 24 : 12, g ? g + 2 * o.m : nullptr};
  }

  SseHead sse_head(const OpDesc& o, bool first_of_level) const {
    if (o.head == 0 && skip_enc_head) return SseHead{};   // (no level map: the epilogue skips the side conv altogether)
    const int acc = first_of_level ? 0 : 1;
    // general head path (classes.hip): the epilogue leaves the side map (acc: consumed by launch_side_to_level)
    if (p.d.n_classes > 1) return SseHead{fat(p.op[&o - kOps].side), nullptr, acc, nullptr, nullptr, 0};
    const HeadSlice hs = head_slice(o);
    return SseHead{nullptr, fat(p.lvl[o.head][kT[o.dst].level]), acc, hs.w, hs.drop, hs.stride};
  }

  // every conv weight of a pass repacked into its MFMA layout by one or two launches (the parameters change every step)
  int pack_all_weights(bool dgrad) {
    if (p.d.conv_impl == SEUNET_CONV_NAIVE) return 0;
    mark("pack_w");
    std::vector<ConvPackJob> jobs;
    std::vector<MarchPackJob> mjobs;
    std::vector<StreamPackJob> sjobs;
    // PyTorch weight w (cout, cin, k,k,k), read transposed / mirrored by the data gradient; src_c -> dst_c: the channels of the
    // conv's source and destination tensors
    const int tf = dgrad ? 1 : 0;
    auto add = [&](ConvKernel k, const float* w, size_t wp, int taps, int cin, int cout, int src_c, int dst_c) {
      if (k == ConvKernel::Stream) sjobs.push_back({w, at(wp), cin, cout, tf, src_c, dst_c});
      else if (k == ConvKernel::March) mjobs.push_back({w, at(wp), cin, cout, tf, src_c, dst_c});
      else jobs.push_back({w, at(wp), taps, cin, cout, tf});
    };
    for (int i = 0; i < kNumOps; ++i) {
      const OpDesc& o = kOps[i];
      if (o.kind != OP_GATED && o.kind != OP_CAT) continue;
      const OpRes& r = p.op[i];
      int ctot = 0;
      for (int k = 0; k < o.nsrc; ++k) ctot += p.C[o.src[k]];
      if (!dgrad) {
        add(r.fwd, par(opp[i].conv1_w), r.wp_f, r.taps, r.cin, r.cout, ctot, r.cout);
        if (o.xname && !p.fuse_x) add(r.x_fwd, par(opp[i].xw), r.wp_x, 1, p.d.in_channel, r.cout, 8, r.cout);
      } else if (r.need_dgrad) {
        add(r.dgrad, par(opp[i].conv1_w), r.wp_d, r.taps, r.cin, r.cout, r.cout, ctot);
      }
    }
    if (!sjobs.empty())
      if (int e = launch_conv_stream_pack_multi(p.d.dtype, sjobs.data(), (int)sjobs.size(), s)) return e;
    if (!mjobs.empty())
      if (int e = launch_conv_march_pack_multi(p.d.dtype, mjobs.data(), (int)mjobs.size(), s)) return e;
    return launch_conv_pack_weights_multi(p.d.dtype, jobs.data(), (int)jobs.size(), s);
  }

  int forward(const float* x, const float* drop1, const float* drop2, float* pred0, float* pred1) {
    skip_enc_head = pred0 == nullptr;
    drops[0] = drop1; drops[1] = drop2;
    if (int e = pack_all_weights(false)) return e;
    mark("pack_input");
    if (int e = launch_pack_input(p.d.dtype, x, p.d.in_channel, at(p.feat[T_X0]), p.dims[0], s)) return e;
    bool lvl_written[2][4] = {{false, false, false, false}, {false, false, false, false}};
    bool pool_done[kNumOps] = {};
    for (int i = 0; i < kNumOps; ++i) {
      const OpDesc& o = kOps[i];
      const OpRes& r = p.op[i];
      const BlockParams& bp = opp[i];
      const int lv = kT[o.dst].level;
      const Dims& dm = p.dims[lv];
      if (o.kind == OP_POOL) {
        if (pool_done[i]) continue;          // written by the aggregation block's epilogue (below)
        mark("pool_fwd:", o.name);
        if (int e = launch_maxpool_fwd(p.d.dtype, at(p.feat[o.src[0]]), p.C[o.src[0]], at(p.feat[o.dst]), p.dims[kT[o.src[0]].level], s)) return e;
      } else if (o.kind == OP_UP) {
        mark("up_fwd:", o.name);
        if (int e = launch_upsample2_fwd(p.d.dtype, at(p.feat[o.src[0]]), p.C[o.src[0]], at(p.feat[o.dst]), p.dims[kT[o.src[0]].level], s)) return e;
      } else if (o.kind == OP_GATED) {
        if (int e = conv_and_stats(o.name, r.fwd, 27, o.dil, srcs(o), r.cin, par(bp.conv1_w), par(bp.conv1_b), r.wp_f, r.raw,
                                   r.cout, r.mean, r.rstd, dm)) return e;
        const SseHead hd = sse_head(o, !lvl_written[o.head][lv]);
        lvl_written[o.head][lv] = true;
        mark("epi_fwd:", o.name);
        if (int e = launch_sse_fwd(p.d.dtype, gate_block(i), at(p.feat[o.dst]), hd, dm, s)) return e;
        if (p.d.n_classes > 1 && hd.side_out != nullptr) {
          const HeadSlice hs = head_slice(o);
          if (int e = launch_side_to_level(fat(r.side), hs.w, hs.stride, hs.drop, hs.stride, p.d.n_classes, fat(p.lvl[o.head][lv]),
                                           hd.level_accumulate, dm, s)) return e;
        }
      } else {  // OP_CAT
        const CatBlock blk = cat_block(i);
        if (int e = conv_and_stats(o.name, r.fwd, 1, 1, srcs(o), r.cin, par(bp.conv1_w), nullptr, r.wp_f, r.raw, r.cout, r.mean,
                                   r.rstd, dm)) return e;
        PoolOut pool_out{};
        if (blk.b.kind == Branch2::Recomputed) {
          // x-branch: statistics from the input's moments, values recomputed inside the epilogue (never stored)
          mark("stats");
          if (int e = launch_xbranch_moments(p.d.dtype, blk.b.src, dat(p.xmom), dm, s)) return e;
          if (int e = launch_xbranch_stats(dat(p.xmom), xbranch_moment_slots(dm), blk.b.w2, r.cout, p.d.in_channel, dm.N, dm.vox(),
                                           p.d.eps, fat(r.mean2), fat(r.rstd2), dat(r.xtot), s)) return e;
          // the max-pool that consumes this block (ec33 -> pool0, ec63 -> pool1, ec93 -> pool2) is written by the same kernel,
          // with the position of each maximum for the backward pass
          const OpDesc& pool = kOps[i + 1];
          SEUNET_CHECK(pool.kind == OP_POOL && pool.src[0] == o.dst && p.op[i + 1].has_pool_idx,
                       "net: internal: %s is not followed by its max-pool", o.name);
          pool_out = PoolOut{at(p.feat[pool.dst]), reinterpret_cast<unsigned*>(at(p.op[i + 1].pool_idx))};
          pool_done[i + 1] = true;
        } else if (blk.b.kind == Branch2::Stored) {
          if (int e = conv_and_stats(o.xname, r.x_fwd, 1, 1, xbranch_src(o), p.d.in_channel, par(bp.xw), nullptr, r.wp_x, r.raw2,
                                     r.cout, r.mean2, r.rstd2, dm)) return e;
        }
        mark("cat_fwd:", o.name);
        if (int e = launch_cat_fwd(p.d.dtype, blk, at(p.feat[o.dst]), pool_out, dm, s)) return e;
      }
    }
    const float* enc[4] = {fat(p.lvl[0][0]), fat(p.lvl[0][1]), fat(p.lvl[0][2]), fat(p.lvl[0][3])};
    const float* dec[3] = {fat(p.lvl[1][0]), fat(p.lvl[1][1]), fat(p.lvl[1][2])};
    mark("head_fwd");
    if (p.d.n_classes > 1) {       // once per (sample, class): level maps [class][N][V], logits (N, K, D, H, W)
      const int K = p.d.n_classes, N = p.d.batch;
      const Dims d1{1, p.dims[0].D, p.dims[0].H, p.dims[0].W};
      for (int hd = 0; hd < 2; ++hd) {
        float* pred = hd == 0 ? pred0 : pred1;
        if (pred == nullptr) continue;
        const int nl = hd == 0 ? 4 : 3;
        for (int n = 0; n < N; ++n)
          for (int c = 0; c < K; ++c) {
            const float* lm[4] = {nullptr, nullptr, nullptr, nullptr};
            for (int l = 0; l < nl; ++l) lm[l] = fat(p.lvl[hd][l]) + ((size_t)c * N + n) * p.dims[l].vox();
            if (int e = launch_head_fwd(lm, nl, par(head_b[hd]) + c, pred + ((size_t)n * K + c) * d1.vox(), d1, s)) return e;
          }
      }
      mark("outside");
      return 0;
    }
    if (!skip_enc_head)
      if (int e = launch_head_fwd(enc, 4, par(head_b[0]), pred0, p.dims[0], s)) return e;
    if (int e = launch_head_fwd(dec, 3, par(head_b[1]), pred1, p.dims[0], s)) return e;
    mark("outside");
    return 0;
  }

  // gradient w.r.t. the raw conv output is in grad[dst]; produce weight gradient and input gradients
  int conv_backward(int i, const SrcList& x, float* const* grads, bool* written) {
    const OpDesc& o = kOps[i];
    const OpRes& r = p.op[i];
    const int lv = kT[o.dst].level;
    const int wi = opp[i].conv1_w;
    if (grads[wi]) {
      mark("wgrad:", o.name);
      if (int e = run_wgrad(r.wgrad, p.d.dtype, r.taps, o.dil, x, r.cin, at(p.grad[o.dst]), r.cout, grads[wi], at(p.wgrad_ws),
                            p.wgrad_ws_bytes, p.dims[lv], s)) return e;
    }
    if (!r.need_dgrad) return 0;
    SrcList gsrc{};
    gsrc.n = 1; gsrc.ptr[0] = at(p.grad[o.dst]); gsrc.C[0] = r.cout;
    DstList gd{};
    gd.n = o.nsrc;
    for (int k = 0; k < o.nsrc; ++k) {
      const int t = o.src[k];
      gd.C[k] = p.C[t];
      gd.ptr[k] = is_input(t) ? nullptr : at(p.grad[t]);
      gd.acc[k] = (!is_input(t) && written[t]) ? 1 : 0;
      if (!is_input(t)) written[t] = true;
    }
    mark("dgrad:", o.name);
    return run_conv(r.dgrad, r.taps, o.dil, gsrc, r.cout, params[wi], 1, at(r.wp_d), nullptr, gd, nullptr, p.dims[lv]);
  }

  hipEvent_t decoder_done = nullptr;   // recorded once every gradient of the decoder blocks (dc1 .. dc6, dc22, dc42) is final

  int backward(const float* g_pred0, const float* g_pred1, const float* drop1, const float* drop2, float* const* grads) {
    drops[0] = drop1; drops[1] = drop2;
    if (int e = pack_all_weights(true)) return e;
    bool written[T_COUNT];
    for (int t = 0; t < T_COUNT; ++t) written[t] = false;
    // heads: level gradients = transposed interpolation of the logit gradients
    {
      mark("head_bwd");
      float* ge[4] = {nullptr, fat(p.glvl[0][1]), fat(p.glvl[0][2]), fat(p.glvl[0][3])};
      float* gd[4] = {nullptr, fat(p.glvl[1][1]), fat(p.glvl[1][2]), nullptr};
      if (p.d.n_classes > 1) {     // once per (sample, class); the bias gradient of a class = its per-sample sums added up
        const int K = p.d.n_classes, N = p.d.batch;
        const Dims d1{1, p.dims[0].D, p.dims[0].H, p.dims[0].W};
        for (int hd = 0; hd < 2; ++hd) {
          const float* gp = hd == 0 ? g_pred0 : g_pred1;
          const int nl = hd == 0 ? 4 : 3;
          for (int n = 0; n < N; ++n)
            for (int c = 0; c < K; ++c) {
              float* gl[4] = {nullptr, nullptr, nullptr, nullptr};
              for (int l = 1; l < nl; ++l) gl[l] = fat(p.glvl[hd][l]) + ((size_t)c * N + n) * p.dims[l].vox();
              if (int e = launch_head_bwd(gp + ((size_t)n * K + c) * d1.vox(), gl, nl, fat(p.head_tmp), fat(p.cls_bias) + n * K + c, d1, s)) return e;
            }
          if (float* gb = grads[head_b[hd]])
            if (int e = launch_class_bias_grad(fat(p.cls_bias), N, K, gb, s)) return e;
        }
      } else {
      if (int e = launch_head_bwd(g_pred0, ge, 4, fat(p.head_tmp), grads[head_b[0]], p.dims[0], s)) return e;
      if (int e = launch_head_bwd(g_pred1, gd, 3, fat(p.head_tmp), grads[head_b[1]], p.dims[0], s)) return e;
      }
    }
    std::vector<float*> zero_ptrs;
    std::vector<int> zero_counts;
    PoolGrad pool_grad[T_COUNT] = {};          // per tensor: a max-pool gradient still to be added by its producer's backward
    for (int i = kNumOps - 1; i >= 0; --i) {
      const OpDesc& o = kOps[i];
      const OpRes& r = p.op[i];
      const BlockParams& bp = opp[i];
      if (decoder_done && strcmp(o.name, "up0") == 0) {
        // the walk is in reverse forward order: everything after up0 (the decoder) has been differentiated.  Its parameter
        // gradients are final from here on (the heads' weights are not: the encoder blocks still add to dc0_0)
        SEUNET_HIP(hipEventRecord(decoder_done, s));
      }
      if (o.kind == OP_POOL || o.kind == OP_UP) {
        const int t = o.src[0];
        if (grad_x && o.dst == T_X2) {
          // pool1x: gx_1 = unpool_1(gx_2), arg-max of the stored X1 (ec63's pass B then adds its own term)
          mark("input_grad:unpool1");
          if (int e = launch_xgrad_unpool(p.d.dtype, at(p.feat[T_X1]), p.d.in_channel, gxl(2), gxl(1), p.dims[1], s)) return e;
        }
        if (is_input(t)) continue;
        SEUNET_CHECK(written[o.dst], "net: internal: gradient of %s output missing", o.name);
        mark(o.kind == OP_POOL ? "pool_bwd:" : "up_bwd:", o.name);
        if (o.kind == OP_POOL) {
          if (r.has_pool_idx) {
            // nothing to launch: the aggregation block that produced tensor t adds this gradient on the fly in both of its
            // backward passes (their PoolGrad argument) -- no read-modify-write of the full-resolution gradient.
            // (dc5, dc3 and dc1 have already differentiated E1, E3 and E5, the tensors these pools read)
            SEUNET_CHECK(written[t], "net: internal: gradient of %s input missing before its deferred pool gradient", o.name);
            pool_grad[t] = PoolGrad{reinterpret_cast<const unsigned*>(at(r.pool_idx)), at(p.grad[o.dst])};
            continue;
          }
          if (int e = launch_maxpool_bwd(p.d.dtype, at(p.feat[t]), at(p.grad[o.dst]), p.C[t], at(p.grad[t]), written[t] ? 1 : 0,
                                         p.dims[kT[t].level], s)) return e;
        } else {
          if (int e = launch_upsample2_bwd(p.d.dtype, at(p.grad[o.dst]), p.C[t], at(p.grad[t]), written[t] ? 1 : 0,
                                           p.dims[kT[t].level], s)) return e;
        }
        written[t] = true;
        continue;
      }
      const int lv = kT[o.dst].level;
      const Dims& dm = p.dims[lv];
      const int P_slots = epi_partials(dm);
      if (o.kind == OP_GATED) {
        const GateBlock blk = gate_block(i);
        SseBwdIn g{written[o.dst] ? at(p.grad[o.dst]) : nullptr, nullptr,
                   lv == 0 ? (o.head == 0 ? g_pred0 : g_pred1) : fat(p.glvl[o.head][lv])};
        SseHead hd = sse_head(o, false);
        const HeadSlice hs = head_slice(o, grads);
        float* g_head = hs.gw;
        if (p.d.n_classes > 1) {
          // general head path: the K level-map gradients of this level folded into the gradient of the block's side map (and the
          // head-weight gradient summed on the way); the block's passes then take g_side
          const int K = p.d.n_classes;
          const long long V = dm.vox();
          const long long cstride = lv == 0 ? V : (long long)dm.N * V, nstride = lv == 0 ? (long long)K * V : V;
          mark("epi_bwd:", o.name);
          if (int e = launch_level_to_side_grad(g.g_level, cstride, nstride, fat(r.side), hs.w, hs.stride, hs.drop, hs.stride, K,
                                                fat(p.gside), dat(p.cls_part), hs.gw, dm, s)) return e;
          g.g_level = nullptr;
          g.g_side = fat(p.gside);
          hd.side_out = nullptr;
          g_head = nullptr;          // (written above; the finalize kernel must not overwrite it)
        }
        mark("epi_bwd:", o.name);   // pass A: f64 sums + parameter-gradient records
        if (int e = launch_sse_bwd_sums(p.d.dtype, blk, g, hd, SseSums{dat(p.stats), fat(p.pgrad)}, dm, s)) return e;
        mark("stats");
        if (int e = launch_gate_bwd_finalize(dat(p.stats), P_slots, r.cout, dm.N, dm.vox(), fat(p.m1), fat(p.m2), fat(p.pgrad),
                                             dm.N * P_slots, grads[bp.se], bp.se2 >= 0 ? grads[bp.se2] : nullptr, grads[bp.conv2_w],
                                             grads[bp.conv2_b], g_head, s)) return e;
        mark("in_bwd:", o.name);    // pass B: recompute dxhat, apply the InstanceNorm backward, store draw over g_e
        if (int e = launch_sse_bwd_apply(p.d.dtype, blk, g, hd, SseApply{fat(p.m1), fat(p.m2), at(p.grad[o.dst])}, dm, s)) return e;
        written[o.dst] = true;
        // conv1.bias feeds an affine-less InstanceNorm: its gradient is identically zero; zeroed in one
        // launch after the loop
        if (float* gb = grads[bp.conv1_b]) { zero_ptrs.push_back(gb); zero_counts.push_back(r.cout); }
        if (int e = conv_backward(i, srcs(o), grads, written)) return e;
      } else {  // OP_CAT
        SEUNET_CHECK(written[o.dst], "net: internal: gradient of %s output missing", o.name);
        const CatBlock blk = cat_block(i);
        const bool two = blk.b.kind != Branch2::None, recomputed = blk.b.kind == Branch2::Recomputed;
        float* gxw = two ? grads[bp.xw] : nullptr;   // the x-branch weight's gradient, if asked for
        const void* g_out = at(p.grad[o.dst]);
        const PoolGrad pool = pool_grad[o.dst];
        mark("cat_bwd:", o.name);   // pass A; a recomputed x-branch also sums what its weight gradient is formed from
        const CatSums sums{dat(p.stats), dat(p.stats2), recomputed && gxw ? dat(p.xwp) : nullptr};
        if (int e = launch_cat_bwd_sums(p.d.dtype, blk, g_out, pool, sums, dm, s)) return e;
        mark("stats");
        if (recomputed && gxw)
          if (int e = launch_cat_xgrad_finalize(dat(p.xwp), dat(p.stats2), P_slots, dat(r.xtot), blk.b.w2, r.cout, p.d.in_channel, dm.N,
                                                p.d.eps, gxw, s)) return e;
        if (int e = launch_stats_finalize(dat(p.stats), P_slots, r.cout, dm.N, dm.vox(), 0.f, 1, fat(p.m1), fat(p.m2), s)) return e;
        if (two)
          if (int e = launch_stats_finalize(dat(p.stats2), P_slots, r.cout, dm.N, dm.vox(), 0.f, 1, fat(p.m1b), fat(p.m2b), s)) return e;
        // pass B: draw over g_out; a stored x-branch's draw goes to gx, a recomputed one adds its input-gradient term on the fly
        mark("in_bwd:", o.name);
        CatApply ap{fat(p.m1), fat(p.m2), fat(p.m1b), fat(p.m2b), at(p.grad[o.dst]), two && !recomputed ? at(p.gx) : nullptr, nullptr, 0};
        if (recomputed && grad_x) { ap.gx_out = gxl(lv); ap.gx_acc = lv == 1 ? 1 : 0; }
        if (int e = launch_cat_bwd_apply(p.d.dtype, blk, g_out, pool, ap, dm, s)) return e;
        if (two && !recomputed) {
          if (grad_x) {   // gx_l (+)= W_x^T d2 from the stored d2 (level 1: on top of unpool_1(gx_2))
            mark("input_grad:", o.xname);
            if (int e = launch_xgrad_contract(p.d.dtype, at(p.gx), r.cout, par(bp.xw), p.d.in_channel, gxl(lv), lv == 1 ? 1 : 0, dm, s)) return e;
          }
          if (gxw) {
            mark("wgrad:", o.xname);
            if (int e = run_wgrad(r.x_wgrad, p.d.dtype, 1, 1, xbranch_src(o), p.d.in_channel, at(p.gx), r.cout, gxw, at(p.wgrad_ws),
                                  p.wgrad_ws_bytes, dm, s)) return e;
          }
        }
        if (int e = conv_backward(i, srcs(o), grads, written)) return e;
      }
    }
    if (!zero_ptrs.empty()) {
      mark("stats");
      if (int e = launch_multi_zero(zero_ptrs.data(), zero_counts.data(), (int)zero_ptrs.size(), s)) return e;
    }
    if (grad_x) {
      // grad_x = convT_ec1(draw_ec1) + gx_0 + unpool_0(gx_1); ec1's pass B left draw_ec1 in grad[T_E0]
      mark("input_grad:ec1");
      if (int e = launch_input_grad(p.d.dtype, at(p.grad[T_E0]), p.C[T_E0], par(opp[0].conv1_w), at(p.feat[T_X0]), p.d.in_channel,
                                    gxl(0), gxl(1), grad_x, p.dims[0], s)) return e;
    }
    mark("outside");
    return 0;
  }
};

}  // namespace
}  // namespace seunet

using namespace seunet;

extern "C" {

int seunet_net_param_count(const seunet_net_desc* desc) {
  if (!desc) return -1;
  return (int)build_registry(*desc).size();
}

int seunet_net_param_info(const seunet_net_desc* desc, int index, char* name, int name_cap, int* shape5, int* ndim) {
  SEUNET_CHECK(desc && name && shape5 && ndim, "param_info: null argument");
  const std::vector<ParamInfo> reg = build_registry(*desc);
  SEUNET_CHECK(index >= 0 && index < (int)reg.size(), "param_info: index %d out of range", index);
  snprintf(name, (size_t)name_cap, "%s", reg[index].name.c_str());
  for (int k = 0; k < 5; ++k) shape5[k] = reg[index].shape[k];
  *ndim = reg[index].ndim;
  return 0;
}

size_t seunet_net_workspace_bytes(const seunet_net_desc* desc) {
  if (!desc) return 0;
  Plan p;
  if (p.init(*desc)) return 0;
  return p.total;
}

int seunet_net_forward(const seunet_net_desc* desc, const float* const* params, const float* x, const float* drop1,
                       const float* drop2, float* pred0, float* pred1, void* workspace, size_t workspace_bytes,
                       seunet_stream_t s) {
  SEUNET_CHECK(x && pred1, "net_forward: null tensor");
  Exec ex;
  if (int e = ex.setup(desc, params, workspace, workspace_bytes, (hipStream_t)s)) return e;
  return ex.forward(x, drop1, drop2, pred0, pred1);
}

// ---- the forward pass as a HIP graph (inference loops call the same forward on the same buffers hundreds of times:
// one graph launch replaces ~150 kernel launches, and the dependent-launch gaps between the small kernels of the coarse
// levels shrink) ----------------------------------------------------------------------------------------------------
struct NetGraph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
};

int seunet_net_forward_capture(const seunet_net_desc* desc, const float* const* params, const float* x, const float* drop1,
                               const float* drop2, float* pred0, float* pred1, void* workspace, size_t workspace_bytes,
                               seunet_stream_t s, void** graph_out) {
  SEUNET_CHECK(x && pred1 && graph_out, "net_forward_capture: null argument");
  SEUNET_CHECK(s != nullptr, "net_forward_capture: stream capture needs a stream other than the null stream");
  SEUNET_CHECK(!prof_on(), "net_forward_capture: switch the launch-group timer off before capturing");
  *graph_out = nullptr;
  Exec ex;
  if (int e = ex.setup(desc, params, workspace, workspace_bytes, (hipStream_t)s)) return e;
  SEUNET_CHECK(device_zero_page() != nullptr, "net_forward_capture: zero page allocation failed");   // (not inside the capture)
  SEUNET_HIP(hipStreamBeginCapture((hipStream_t)s, hipStreamCaptureModeThreadLocal));
  const int rc = ex.forward(x, drop1, drop2, pred0, pred1);
  NetGraph* g = new NetGraph;
  const hipError_t e_end = hipStreamEndCapture((hipStream_t)s, &g->graph);
  if (rc != 0 || e_end != hipSuccess) {
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
    if (rc != 0) return rc;    // (the message of the failing launch is already recorded)
    return fail("net_forward_capture: hipStreamEndCapture failed: %s", hipGetErrorString(e_end));
  }
  const hipError_t e_inst = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
  if (e_inst != hipSuccess) {
    (void)hipGraphDestroy(g->graph);
    delete g;
    return fail("net_forward_capture: hipGraphInstantiate failed: %s", hipGetErrorString(e_inst));
  }
  *graph_out = g;
  return 0;
}

int seunet_graph_launch(void* graph, seunet_stream_t s) {
  SEUNET_CHECK(graph != nullptr, "graph_launch: null graph");
  SEUNET_HIP(hipGraphLaunch(static_cast<NetGraph*>(graph)->exec, (hipStream_t)s));
  return 0;
}

int seunet_graph_destroy(void* graph) {
  if (!graph) return 0;
  NetGraph* g = static_cast<NetGraph*>(graph);
  if (g->exec) (void)hipGraphExecDestroy(g->exec);
  if (g->graph) (void)hipGraphDestroy(g->graph);
  delete g;
  return 0;
}

// Diagnostic read-back of one intermediate of the LAST forward that ran on `workspace` (nothing is recomputed): which = 0 the
// raw conv output of block `name` (before InstanceNorm; NCDHW f32, `channels` of them), 1 / 2 its per-(n, c) mean / rstd
// ([N][C] f32), 3 the block's output tensor (for an aggregation block: after the x-branch was added; NCDHW f32).  Used by the
// flip census (tests/flip_census.py): LeakyReLU sign / max-pool argmax disagreements with the float64 oracle.
int seunet_net_read_tensor(const seunet_net_desc* desc, const float* const* params, const void* workspace, size_t workspace_bytes,
                           const char* name, int which, float* out, int* channels, seunet_stream_t s) {
  SEUNET_CHECK(desc && workspace && name && out, "net_read_tensor: null argument");
  Plan p;
  if (int e = p.init(*desc)) return e;
  SEUNET_CHECK(workspace_bytes >= p.total, "net_read_tensor: workspace too small");
  const unsigned char* ws = reinterpret_cast<const unsigned char*>(workspace);
  for (int i = 0; i < kNumOps; ++i) {
    const OpDesc& o = kOps[i];
    if (o.kind != OP_GATED && o.kind != OP_CAT) continue;
    const OpRes& r = p.op[i];
    const int lv = kT[o.dst].level;
    if (o.xname && std::string(o.xname) == name) {   // the raw-input branch of an aggregation block, when it is materialised (in_channel > 2)
      SEUNET_CHECK(which >= 0 && which <= 2, "net_read_tensor: which=%d is not stored for an x-branch", which);
      if (channels) *channels = r.cout;
      if (which == 0 && p.fuse_x) {
        // in_channel <= 2: the branch is recomputed inside the aggregation epilogue and leaves no tensor: recompute it here by the
        // same device function, from the packed input in the workspace and the caller's weights
        SEUNET_CHECK(params != nullptr, "net_read_tensor: the recomputed x-branch %s needs the parameter list", name);
        BlockParams blocks[kNumBlocks];
        build_registry(p.d, blocks);
        const int wi = blocks[find_block(o.xname)].conv1_w;
        SEUNET_CHECK(params[wi], "net_read_tensor: no weight for %s", name);
        return launch_xbranch_values(p.d.dtype, ws + p.feat[o.xsrc], params[wi], r.cout, p.d.in_channel, out, p.dims[lv], (hipStream_t)s);
      }
      if (which == 0) return launch_unpack_cl(p.d.dtype, ws + r.raw2, r.cout, out, p.dims[lv], (hipStream_t)s);
      SEUNET_HIP(hipMemcpyAsync(out, ws + (which == 1 ? r.mean2 : r.rstd2), (size_t)p.d.batch * r.cout * 4, hipMemcpyDeviceToDevice, (hipStream_t)s));
      return 0;
    }
    if (std::string(o.name) != name) continue;
    if (channels) *channels = which == 3 ? p.C[o.dst] : r.cout;
    if (which == 0) return launch_unpack_cl(p.d.dtype, ws + r.raw, r.cout, out, p.dims[lv], (hipStream_t)s);
    if (which == 3) return launch_unpack_cl(p.d.dtype, ws + p.feat[o.dst], p.C[o.dst], out, p.dims[lv], (hipStream_t)s);
    SEUNET_CHECK(which == 1 || which == 2, "net_read_tensor: which=%d", which);
    SEUNET_HIP(hipMemcpyAsync(out, ws + (which == 1 ? r.mean : r.rstd), (size_t)p.d.batch * r.cout * 4, hipMemcpyDeviceToDevice, (hipStream_t)s));
    return 0;
  }
  return fail("net_read_tensor: no block named %s", name);
}

static_assert((int)ConvKernel::Naive == SEUNET_KERNEL_NAIVE && (int)ConvKernel::Tiled == SEUNET_KERNEL_TILED &&
                  (int)ConvKernel::Stream == SEUNET_KERNEL_STREAM && (int)ConvKernel::March == SEUNET_KERNEL_MARCH &&
                  (int)ConvKernel::Wgrad1x1 == SEUNET_KERNEL_WGRAD1X1,
              "SEUNET_KERNEL_* are the values of ConvKernel");

int seunet_net_conv_info(const seunet_net_desc* desc, int index, seunet_conv_info* out) {
  SEUNET_CHECK(desc && out, "net_conv_info: null argument");
  Plan p;
  if (int e = p.init(*desc)) return e;
  SEUNET_CHECK(index >= 0, "net_conv_info: index %d out of range", index);
  int seen = 0;
  for (int i = 0; i < kNumOps; ++i) {
    const OpDesc& o = kOps[i];
    if (o.kind != OP_GATED && o.kind != OP_CAT) continue;
    if (seen++ != index) continue;
    const OpRes& r = p.op[i];
    const int lv = kT[o.dst].level;
    *out = seunet_conv_info{};
    snprintf(out->name, sizeof out->name, "%s", o.name);
    out->taps = r.taps;
    out->dilation = o.kind == OP_GATED ? o.dil : 1;
    out->level = lv;
    out->dims = seunet_dims{p.dims[lv].N, p.dims[lv].D, p.dims[lv].H, p.dims[lv].W};
    out->nsrc = o.nsrc;
    for (int k = 0; k < o.nsrc; ++k) { out->src_c[k] = p.C[o.src[k]]; out->src_is_input[k] = is_input(o.src[k]) ? 1 : 0; }
    out->cin = r.cin;
    out->cout = r.cout;
    out->need_dgrad = r.need_dgrad ? 1 : 0;
    out->fwd = (int)r.fwd;
    out->dgrad = (int)r.dgrad;
    out->wgrad = (int)r.wgrad;
    if (o.xname) {
      snprintf(out->x_name, sizeof out->x_name, "%s", o.xname);
      out->x_materialised = p.fuse_x ? 0 : 1;
      out->x_fwd = (int)r.x_fwd;
      out->x_wgrad = (int)r.x_wgrad;
    }
    out->src_dist = o.nsrc == 2 ? (long long)p.feat[o.src[1]] - (long long)p.feat[o.src[0]] : 0;
    return 0;
  }
  return fail("net_conv_info: index %d is past the last convolution (%d)", index, seen);
}

int seunet_net_backward(const seunet_net_desc* desc, const float* const* params, const float* g_pred0,
                        const float* g_pred1, const float* drop1, const float* drop2, float* const* grads,
                        void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  return seunet_net_backward_ev(desc, params, g_pred0, g_pred1, drop1, drop2, grads, workspace, workspace_bytes, s, nullptr);
}

int seunet_net_backward_ev(const seunet_net_desc* desc, const float* const* params, const float* g_pred0,
                           const float* g_pred1, const float* drop1, const float* drop2, float* const* grads,
                           void* workspace, size_t workspace_bytes, seunet_stream_t s, void* decoder_done_event) {
  SEUNET_CHECK(g_pred0 && g_pred1 && grads, "net_backward: null tensor");
  Exec ex;
  if (int e = ex.setup(desc, params, workspace, workspace_bytes, (hipStream_t)s)) return e;
  ex.decoder_done = reinterpret_cast<hipEvent_t>(decoder_done_event);
  return ex.backward(g_pred0, g_pred1, drop1, drop2, grads);
}

size_t seunet_net_input_grad_bytes(const seunet_net_desc* desc) {
  if (!desc) { (void)fail("net_input_grad_bytes: null descriptor"); return 0; }
  Plan p;
  if (p.init(*desc)) return 0;
  return p.ig_total;
}

int seunet_net_backward_input(const seunet_net_desc* desc, const float* const* params, const float* g_pred0, const float* g_pred1,
                              const float* drop1, const float* drop2, float* const* grads, float* grad_x, void* scratch,
                              size_t scratch_bytes, void* workspace, size_t workspace_bytes, seunet_stream_t s,
                              void* decoder_done_event) {
  if (grad_x == nullptr)
    return seunet_net_backward_ev(desc, params, g_pred0, g_pred1, drop1, drop2, grads, workspace, workspace_bytes, s, decoder_done_event);
  SEUNET_CHECK(g_pred0 && g_pred1 && grads && scratch, "net_backward_input: null tensor");
  Exec ex;
  if (int e = ex.setup(desc, params, workspace, workspace_bytes, (hipStream_t)s)) return e;
  SEUNET_CHECK(scratch_bytes >= ex.p.ig_total, "net_backward_input: scratch too small (%zu < %zu bytes)", scratch_bytes, ex.p.ig_total);
  SEUNET_CHECK((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "net_backward_input: scratch must be 256-byte aligned");
  ex.decoder_done = reinterpret_cast<hipEvent_t>(decoder_done_event);
  ex.grad_x = grad_x;
  ex.igs = reinterpret_cast<unsigned char*>(scratch);
  return ex.backward(g_pred0, g_pred1, drop1, drop2, grads);
}

}  // extern "C"
