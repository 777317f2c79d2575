// Whole-network executor: SE_UNet.forward (reference SE_UNet.py:181-238) and its backward, as one
// stream-ordered sequence of the kernels in this directory.  The graph is data (kOps below, the only hand-written description
// of the network; everything else about it is derived once, kG) and two small interpreters walk it forwards / backwards, one
// member function per op kind and direction; nothing here allocates device memory: every intermediate lives at a fixed
// offset of a caller-owned workspace whose layout is a pure function of seunet_net_desc (so the same
// layout is recomputed by the backward call).
#include "seunet_common.h"
#include "epilogue.h"
#include "wgrad.h"
#include "../../include/seunet_hip.h"

#include <algorithm>
#include <cstdio>
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

// diagnostic switch (seunet_debug_net_wgrad_defer): off = every weight gradient of the backward walk reduces its slabs at once
bool g_wgrad_defer = true;

// ---------------------------------------------------------------------------------------------------
// the graph
// ---------------------------------------------------------------------------------------------------
enum TId {
  T_NONE,   // ends a row's source list
  T_X0, T_X1, T_X2,
  T_E0, T_E1A, T_E1_1, T_E1, T_E2IN, T_E2, T_E3A, T_E3_1, T_E3, T_E4IN, T_E4, T_E5A, T_E5_1, T_E5,
  T_E6IN, T_E6, T_E7A, T_E7_1, T_E7, T_E8, T_D0A, T_D0_1, T_D0, T_D1U, T_D1A, T_D1_1, T_D1, T_D2U, T_D2A, T_D2_1,
  T_COUNT
};
enum OpKind { OP_GATED, OP_CAT, OP_POOL, OP_UP };
struct OpDesc {
  OpKind kind; const char* name;
  int src[3]; int dst;
  int cout;                      // gated / aggregation: output channels at width 1
  int dil; int gates;            // gated: dilation, #gates
  const char* xname; int xsrc;   // aggregation: optional raw-input branch
};
constexpr OpDesc kOps[] = {
    {.kind = OP_GATED, .name = "ec1", .src = {T_X0}, .dst = T_E0, .cout = 8, .dil = 1, .gates = 1},
    {.kind = OP_GATED, .name = "ec2", .src = {T_E0}, .dst = T_E1A, .cout = 16, .dil = 1, .gates = 1},
    {.kind = OP_GATED, .name = "ec3", .src = {T_E1A}, .dst = T_E1_1, .cout = 32, .dil = 2, .gates = 1},
    {.kind = OP_CAT, .name = "ec33", .src = {T_E1_1, T_E0, T_E1A}, .dst = T_E1, .cout = 32, .xname = "x33", .xsrc = T_X0},
    {.kind = OP_POOL, .name = "pool0", .src = {T_E1}, .dst = T_E2IN},
    {.kind = OP_POOL, .name = "pool0x", .src = {T_X0}, .dst = T_X1},
    {.kind = OP_GATED, .name = "ec4", .src = {T_E2IN}, .dst = T_E2, .cout = 32, .dil = 1, .gates = 2},
    {.kind = OP_GATED, .name = "ec5", .src = {T_E2}, .dst = T_E3A, .cout = 32, .dil = 2, .gates = 2},
    {.kind = OP_GATED, .name = "ec6", .src = {T_E3A}, .dst = T_E3_1, .cout = 64, .dil = 2, .gates = 2},
    {.kind = OP_CAT, .name = "ec63", .src = {T_E3_1, T_E2, T_E3A}, .dst = T_E3, .cout = 64, .xname = "x63", .xsrc = T_X1},
    {.kind = OP_POOL, .name = "pool1", .src = {T_E3}, .dst = T_E4IN},
    {.kind = OP_POOL, .name = "pool1x", .src = {T_X1}, .dst = T_X2},
    {.kind = OP_GATED, .name = "ec7", .src = {T_E4IN}, .dst = T_E4, .cout = 64, .dil = 1, .gates = 2},
    {.kind = OP_GATED, .name = "ec8", .src = {T_E4}, .dst = T_E5A, .cout = 64, .dil = 2, .gates = 2},
    {.kind = OP_GATED, .name = "ec9", .src = {T_E5A}, .dst = T_E5_1, .cout = 64, .dil = 2, .gates = 2},
    {.kind = OP_CAT, .name = "ec93", .src = {T_E5_1, T_E4, T_E5A}, .dst = T_E5, .cout = 64, .xname = "x93", .xsrc = T_X2},
    {.kind = OP_POOL, .name = "pool2", .src = {T_E5}, .dst = T_E6IN},
    {.kind = OP_GATED, .name = "ec10", .src = {T_E6IN}, .dst = T_E6, .cout = 64, .dil = 1, .gates = 2},
    {.kind = OP_GATED, .name = "ec11", .src = {T_E6}, .dst = T_E7A, .cout = 64, .dil = 1, .gates = 2},
    {.kind = OP_GATED, .name = "ec12", .src = {T_E7A}, .dst = T_E7_1, .cout = 64, .dil = 1, .gates = 2},
    {.kind = OP_CAT, .name = "ec123", .src = {T_E7_1, T_E6, T_E7A}, .dst = T_E7, .cout = 64},
    {.kind = OP_UP, .name = "up0", .src = {T_E7}, .dst = T_E8},
    {.kind = OP_GATED, .name = "dc1", .src = {T_E8, T_E5}, .dst = T_D0A, .cout = 64, .dil = 1, .gates = 2},
    {.kind = OP_GATED, .name = "dc2", .src = {T_D0A}, .dst = T_D0_1, .cout = 64, .dil = 1, .gates = 2},
    {.kind = OP_CAT, .name = "dc22", .src = {T_D0_1, T_D0A}, .dst = T_D0, .cout = 64},
    {.kind = OP_UP, .name = "up1", .src = {T_D0}, .dst = T_D1U},
    {.kind = OP_GATED, .name = "dc3", .src = {T_D1U, T_E3}, .dst = T_D1A, .cout = 64, .dil = 1, .gates = 2},
    {.kind = OP_GATED, .name = "dc4", .src = {T_D1A}, .dst = T_D1_1, .cout = 32, .dil = 1, .gates = 2},
    {.kind = OP_CAT, .name = "dc42", .src = {T_D1_1, T_D1A}, .dst = T_D1, .cout = 32},
    {.kind = OP_UP, .name = "up2", .src = {T_D1}, .dst = T_D2U},
    {.kind = OP_GATED, .name = "dc5", .src = {T_D2U, T_E1}, .dst = T_D2A, .cout = 32, .dil = 1, .gates = 1},
    {.kind = OP_GATED, .name = "dc6", .src = {T_D2A}, .dst = T_D2_1, .cout = 16, .dil = 1, .gates = 1},
    // dc62 (SE_UNet.py:148,230) is dead: never evaluated, no gradient; Graph::derive gives it its registry entry
};
constexpr int kNumOps = sizeof(kOps) / sizeof(kOps[0]);
constexpr bool is_conv(const OpDesc& o) { return o.kind == OP_GATED || o.kind == OP_CAT; }

// ---------------------------------------------------------------------------------------------------
// what follows from kOps, derived once (kG): tensor levels and channels, each block's input channels, the two heads
// and the parameter registry == the reference's state_dict order (SE_UNet.py:108-151)
// ---------------------------------------------------------------------------------------------------
enum PField { P_CONV1_W, P_CONV1_B, P_CONV2_W, P_CONV2_B, P_SE, P_SE2, P_HEAD_W, P_HEAD_B };
constexpr const char* kFieldName[] = {"conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv_se.weight", "conv_se2.weight",
                                      "weight", "bias"};
// registry indices of a block's parameters by PField, -1 = none; xw: the weight of an aggregation block's x-branch (x33 / x63 / x93)
struct BlockParams { int at[6] = {-1, -1, -1, -1, -1, -1}, xw = -1; };
// channels at width 1, cin 0 = in_channel (a head's cin: its side channels at any width); k: extent of conv1's kernel
struct ParamDesc { const char* block; PField f; int cin, cout, k; };
constexpr int kNumParams = 117;   // DESIGN.md; SURVEY 2.3

struct Graph {
  int level[T_COUNT] = {}, cbase[T_COUNT] = {};   // per tensor; cbase: channels at width 1, 0 = the padded network input (8 channels)
  const char* tname[T_COUNT] = {};                // named after the op that writes it
  int nsrc[kNumOps] = {}, cin[kNumOps] = {};      // conv ops: sum of the sources' cbase (0: in_channel)
  int head[kNumOps] = {}, slot[kNumOps] = {};     // gated ops: 0 = encoder head (before the first up-sampling) / 1 = decoder head; ordinal within it
  int sides[2] = {};                              // gated ops per head: each feeds 2 side channels
  int first_up = -1, nconv = 0;
  BlockParams prm[kNumOps] = {};
  ParamDesc param[kNumParams] = {};
  int nparams = 0, dead = -1, head_w[2] = {}, head_b[2] = {};   // dead: dc62's weight, which no caller need pass

  constexpr int add(const char* block, PField f, int ci, int co, int k) { param[nparams] = {block, f, ci, co, k}; return nparams++; }
  constexpr BlockParams add_block(const char* name, int gates, int ci, int co) {
    BlockParams b;
    const int fields = gates ? 4 + gates : 1;   // an aggregation block has conv1.weight alone; a gated one up to conv_se / conv_se2
    for (int f = 0; f < fields; ++f) b.at[f] = add(name, (PField)f, ci, co, gates ? 3 : 1);
    return b;
  }
};
constexpr Graph derive() {
  Graph g;
  g.tname[T_X0] = "x";
  for (int i = 0; i < kNumOps; ++i) {
    const OpDesc& o = kOps[i];
    for (int k = 0; k < 3 && o.src[k] != T_NONE; ++k) { ++g.nsrc[i]; g.cin[i] += g.cbase[o.src[k]]; }
    g.level[o.dst] = g.level[o.src[0]] + (o.kind == OP_POOL) - (o.kind == OP_UP);
    g.cbase[o.dst] = is_conv(o) ? o.cout : g.cbase[o.src[0]];
    g.tname[o.dst] = o.name;
    if (o.kind == OP_UP && g.first_up < 0) g.first_up = i;
    if (o.kind == OP_GATED) { g.head[i] = g.first_up >= 0; g.slot[i] = g.sides[g.head[i]]++; }
    if (!is_conv(o)) continue;
    ++g.nconv;
    // registry order: walk order, each x-branch after its aggregation block
    g.prm[i] = g.add_block(o.name, o.gates, g.cin[i], o.cout);
    if (o.xname) g.prm[i].xw = g.add_block(o.xname, 0, 0, o.cout).at[P_CONV1_W];
  }
  g.dead = g.add_block("dc62", 0, 48, 16).at[P_CONV1_W];
  for (int h = 0; h < 2; ++h) {
    g.head_w[h] = g.add(h ? "dc0_1" : "dc0_0", P_HEAD_W, 2 * g.sides[h], 0, 1);
    g.head_b[h] = g.add(h ? "dc0_1" : "dc0_0", P_HEAD_B, 0, 0, 0);
  }
  return g;
}
constexpr Graph kG = derive();
static_assert(2 * kG.sides[0] == 24 && 2 * kG.sides[1] == 12, "dc0_0 takes 24 side channels, dc0_1 12 (SE_UNet.py:150-151)");
static_assert(kG.nparams == kNumParams, "the reference's state_dict has 117 tensors");

constexpr bool is_input(int t) { return kG.cbase[t] == 0; }

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
  // an aggregation block with a recomputed x-branch, whose epilogue also writes the max-pool of its output, and that pool: each
  // other's op index (resolved in Plan::init), else -1.  The pool then holds the arg-max words of the forward, and launches nothing itself
  int fused = -1;
  size_t pool_idx = 0;
  size_t side = 0;                                             // n_classes > 1: the block's 2-channel side map, f32 [N][V][2] (classes.hip)
};

// one buffer of the plan, for seunet_debug_net_layout: "what:of" (the take of a tensor or block `of`), or "what"
struct Take { const char* what; const char* of; size_t off, bytes; };
constexpr const char* kDigit[] = {"0", "1", "2", "3"};

struct Plan {
  seunet_net_desc d;
  size_t esz;
  Dims dims[4];
  int C[T_COUNT];
  size_t feat[T_COUNT], grad[T_COUNT];
  OpRes op[kNumOps];
  size_t lvl[2][4], glvl[2][4];
  size_t stats, stats2, pgrad, m1, m2, m1b, m2b, wgrad_ws, head_tmp, gx, xwp = 0, xmom = 0;
  size_t gside = 0, cls_part = 0, cls_bias = 0;                // n_classes > 1: side-map gradient of one block, head-gradient records, per-(sample, class) bias sums
  // x-branches (x33 / x63 / x93) recomputed from the <= 2-channel input instead of materialised (csrc/cat.hip, XR)
  bool fuse_x = false;
  size_t wgrad_ws_bytes;
  size_t total;
  // input gradient (seunet_net_backward_input): a SEPARATE caller-owned scratch buffer, laid out here so that the workspace (and
  // seunet_net_workspace_bytes) stays what it is -- the per-level x-branch terms gx_l = W_xl^T d2_xl, f32 [N][V_l][in_channel].
  // Carved (and logged, under "ig:" names) after the workspace's buffers, from offset 0 again
  size_t ig_gx[3] = {0, 0, 0}, ig_total = 0;

  // bump carver of the workspace (volume.h has the device-pointer sibling, WsCarver); every take is logged in order
  size_t cur = 0;
  std::vector<Take> log;
  size_t take(size_t bytes, const char* what, const char* of = "") {
    log.push_back({what, of, cur, bytes});
    cur = align_up(cur + bytes, 256);
    return log.back().off;
  }

  const Dims& dims_of(int t) const { return dims[kG.level[t]]; }
  // byte distance of a two-source block's sources (the marching weight gradient reaches both sources of dc5 through one 32-bit
  // descriptor: their distance counts)
  long long src_dist(int i) const {
    return kG.nsrc[i] == 2 ? (long long)feat[kOps[i].src[1]] - (long long)feat[kOps[i].src[0]] : 0;
  }

  // The kernel of every conv pass of op i (OpRes::fwd .. x_wgrad).
  void route(int i) {
    const OpDesc& o = kOps[i];
    OpRes& r = op[i];
    if (d.conv_impl == SEUNET_CONV_NAIVE) { r.fwd = r.dgrad = r.wgrad = r.x_fwd = r.x_wgrad = ConvKernel::Naive; return; }
    const Dims& dm = dims_of(o.dst);
    SrcList x{}, gy{};   // the forward's sources and the data gradient's
    DstList y{}, gx{};   // and their destinations
    x.n = gx.n = kG.nsrc[i];
    for (int k = 0; k < x.n; ++k) x.C[k] = gx.C[k] = C[o.src[k]];
    y.n = gy.n = 1;
    y.C[0] = gy.C[0] = r.cout;
    const int c0 = C[o.src[0]];
    // small-channel 3x3x3 layers with one source tensor (ec1 / ec2 / ec3 / dc6 at width 1) run on the streaming kernel
    // (the streaming kernels address one sample through 32-bit buffer offsets; a sample of 4 GB or more takes the general kernels)
    const bool stream_ok = o.kind == OP_GATED && x.n == 1 && (long long)dm.D * dm.H * dm.W * 32 * (long long)esz < 0xFFFFFFFFll;
    const bool stream_f = stream_ok && conv_supported(ConvKernel::Stream, d.dtype, 27, o.dil, x, y);
    const bool stream_d = stream_ok && conv_supported(ConvKernel::Stream, d.dtype, 27, o.dil, gy, gx);
    // 32 / 64-input-channel 3x3x3 layers of the levels that fill the chip with 32-voxel rows run on the marching kernel
    // (one workgroup per CU, weights in registers): dc5, dc4, ec4..ec6 and the data gradients of those and of dc3
    const bool march_ok = o.kind == OP_GATED && !stream_f && march_level(dm, o.dil);
    r.fwd = stream_f ? ConvKernel::Stream
          : march_ok && conv_supported(ConvKernel::March, d.dtype, 27, o.dil, x, y) ? ConvKernel::March : ConvKernel::Tiled;
    r.dgrad = stream_d ? ConvKernel::Stream
            : march_ok && conv_supported(ConvKernel::March, d.dtype, 27, o.dil, gy, gx) ? ConvKernel::March : ConvKernel::Tiled;
    r.wgrad = stream_ok && wgrad_stream_supported(d.dtype, 27, o.dil, c0, r.cout)
                  ? ConvKernel::Stream : wgrad_kernel(d.dtype, r.taps, o.dil, x, r.cin, r.cout, dm, src_dist(i));
    if (o.xname) {   // the x-branch: 1x1x1 conv of the 8-channel padded input
      const SrcList xs{{}, {8}, 1};
      r.x_fwd = ConvKernel::Tiled;
      r.x_wgrad = wgrad_kernel(d.dtype, 1, 1, xs, d.in_channel, r.cout, dm, 0);
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
    log.reserve(320);
    for (int l = 0; l < 4; ++l) dims[l] = Dims{d.batch, d.d >> l, d.h >> l, d.w >> l};
    for (int t = T_X0; t < T_COUNT; ++t) C[t] = is_input(t) ? 8 : kG.cbase[t] * d.width_mult;
    auto tensor_bytes = [&](int t) { return (size_t)d.batch * dims_of(t).vox() * C[t] * esz; };
    // (the two sources of a two-source marching layer are allocated next to each other: the kernel then reaches both through one
    // 32-bit buffer descriptor, conv_march.hip `BUF` and wgrad_march.hip)
    // (dc5 only: T_D2U right after T_E1.  The same placement for dc3 and dc1 cost their tiled forward 5 % -- conv_fwd:dc3
    // 0.465 -> 0.49 ms, same box, alternating runs -- and their sources are 1.2 GB apart at batch 4 anyway; beyond 4 GB the weight
    // gradient of those two layers takes the tiled kernel)
    static_assert(T_E1 < T_D2U, "the mate is placed before the walk reaches it");
    for (int t = T_X0; t < T_COUNT; ++t) {
      if (t != T_D2U) feat[t] = take(tensor_bytes(t), "out", kG.tname[t]);
      if (t == T_E1) feat[T_D2U] = take(tensor_bytes(T_D2U), "out", kG.tname[T_D2U]);
      grad[t] = is_input(t) ? 0 : take(tensor_bytes(t), "grad", kG.tname[t]);
    }
    size_t gx_max = 0, wg_max = 0, xw_max = 0, xmom_max = 0;
    fuse_x = d.in_channel <= 2 && d.conv_impl != SEUNET_CONV_NAIVE;
    int slots_max = 1, cmax = 8;
    for (int i = 0; i < kNumOps; ++i) {
      const OpDesc& o = kOps[i];
      OpRes& r = op[i];
      for (int c = 0; c < i && o.kind == OP_POOL && fuse_x; ++c) {
        if (kOps[c].kind != OP_CAT || !kOps[c].xname || kOps[c].dst != o.src[0]) continue;
        // the forward of aggregation block c writes this pool (and the position of each maximum, which the backward pass then
        // reads instead of the block output and the pooled tensor)
        r.pool_idx = take((size_t)d.batch * dims_of(o.dst).vox() * (C[o.src[0]] / 8) * 4, "argmax", o.name);
        r.fused = c;
        op[c].fused = i;
      }
      if (!is_conv(o)) continue;
      const Dims& dm = dims_of(o.dst);
      r.cout = C[o.dst];
      r.taps = o.kind == OP_GATED ? 27 : 1;
      r.cin = kG.cin[i] ? kG.cin[i] * d.width_mult : d.in_channel;
      r.need_dgrad = kG.cin[i] != 0;   // (none towards the network input)
      const size_t act = tensor_bytes(o.dst);
      r.raw = take(act, "raw", o.name);
      r.mean = take((size_t)d.batch * r.cout * 4, "mean", o.name);
      r.rstd = take((size_t)d.batch * r.cout * 4, "rstd", o.name);
      route(i);
      r.wp_f = take(conv_wpack_bytes(r.fwd, d.dtype, r.taps, C[o.src[0]], r.cin, r.cout), "wp_f", o.name);
      if (r.need_dgrad) r.wp_d = take(conv_wpack_bytes(r.dgrad, d.dtype, r.taps, r.cout, r.cout, r.cin), "wp_d", o.name);
      slots_max = std::max(slots_max, conv_slots(r.fwd, dm, r.taps, o.dil, r.cin, r.cout));
      if (r.wgrad == ConvKernel::Stream) wg_max = std::max(wg_max, wgrad_stream_workspace_bytes(C[o.src[0]], r.cout, o.dil, dm));
      wg_max = std::max(wg_max, wgrad_workspace_bytes(r.taps, r.cin, r.cout));
      if (o.xname) {
        r.mean2 = take((size_t)d.batch * r.cout * 4, "mean", o.xname);
        r.rstd2 = take((size_t)d.batch * r.cout * 4, "rstd", o.xname);
        if (fuse_x) {
          xw_max = std::max(xw_max, (size_t)d.batch * epi_partials(dm) * r.cout * 2 * 8);
          r.xtot = take((size_t)d.batch * 5 * 8, "xtot", o.xname);      // the input's moments per sample, kept for the backward pass
          xmom_max = std::max(xmom_max, (size_t)d.batch * xbranch_moment_slots(dm) * 5 * 8);
        } else {
          r.raw2 = take(act, "raw", o.xname);
          r.wp_x = take(conv_wpack_bytes(r.x_fwd, d.dtype, 1, 8, d.in_channel, r.cout), "wp_f", o.xname);
          gx_max = std::max(gx_max, act);
          wg_max = std::max(wg_max, wgrad_workspace_bytes(1, d.in_channel, r.cout));
        }
      }
      slots_max = std::max(slots_max, std::max(std::max(conv_stats_tiles(dm, 27, 1), conv_stats_tiles(dm, 27, 2)), epi_partials(dm)));
      cmax = std::max(cmax, r.cout);
      if (d.n_classes > 1 && o.kind == OP_GATED) r.side = take((size_t)d.batch * dm.vox() * 2 * 4, "side", o.name);
    }
    for (int h = 0; h < 2; ++h)
      for (int l = 0; l < 4; ++l) {
        lvl[h][l] = take((size_t)d.n_classes * d.batch * dims[l].vox() * 4, h ? "lvl.dec" : "lvl.enc", kDigit[l]);       // [class][N][V]
        glvl[h][l] = take((size_t)d.n_classes * d.batch * dims[l].vox() * 4, h ? "glvl.dec" : "glvl.enc", kDigit[l]);
      }
    if (d.n_classes > 1) {
      gside = take((size_t)d.batch * dims[0].vox() * 2 * 4, "gside");
      cls_part = take((size_t)d.batch * 256 * 2 * d.n_classes * 8, "cls_part");
      cls_bias = take((size_t)d.batch * d.n_classes * 4, "cls_bias");
    }
    const size_t stat_bytes = (size_t)d.batch * slots_max * cmax * 2 * 8;   // f32 forward / f64 backward partials
    stats = take(stat_bytes, "stats");
    stats2 = take(stat_bytes, "stats2");
    pgrad = take((size_t)d.batch * slots_max * (4 * cmax + 4) * 4, "pgrad");
    m1 = take((size_t)d.batch * cmax * 4, "m1");
    m2 = take((size_t)d.batch * cmax * 4, "m2");
    m1b = take((size_t)d.batch * cmax * 4, "m1b");
    m2b = take((size_t)d.batch * cmax * 4, "m2b");
    wgrad_ws_bytes = wg_max;
    wgrad_ws = take(wg_max, "wgrad_ws");
    head_tmp = take(head_bwd_tmp_floats(dims[0]) * 4, "head_tmp");
    gx = take(gx_max, "gx");
    xwp = take(xw_max, "xwp");
    xmom = take(xmom_max, "xmom");
    total = cur;
    cur = 0;
    for (int l = 0; l < 3; ++l) ig_gx[l] = take((size_t)d.batch * dims[l].vox() * d.in_channel * 4, "ig:gx", kDigit[l]);
    ig_total = cur;
    return 0;
  }
};

// The plan of a descriptor and one of its conv ops, for the host-side queries: the index-th conv of the walk (name null), or the
// block of that name, or the aggregation block whose x-branch has that name (*xbranch).  *op = -1: there is none
int plan_and_find(const seunet_net_desc& desc, int index, const char* name, Plan* p, int* op, bool* xbranch = nullptr) {
  if (int e = p->init(desc)) return e;
  *op = -1;
  for (int i = 0, seen = 0; i < kNumOps && *op < 0; ++i) {
    const OpDesc& o = kOps[i];
    if (!is_conv(o)) continue;
    const bool is_x = name && o.xname && strcmp(o.xname, name) == 0;
    if (name ? is_x || strcmp(o.name, name) == 0 : seen++ == index) { *op = i; if (xbranch) *xbranch = is_x; }
  }
  return 0;
}

struct Exec {
  Plan p;
  unsigned char* ws = nullptr;
  const float* const* params = nullptr;
  hipStream_t s = nullptr;
  float* grad_x = nullptr;             // seunet_net_backward_input: NCDHW f32 input gradient (null = not requested)
  unsigned char* igs = nullptr;        // its scratch buffer (Plan::ig_gx)
  const float* drops[2] = {nullptr, nullptr};   // DropLayer scales of the encoder / decoder head, or null

  float* gxl(int l) const { return reinterpret_cast<float*>(igs + p.ig_gx[l]); }
  void mark(const char* tag, const char* name = "") const { if (prof_on()) prof_mark((std::string(tag) + name).c_str(), s); }
  void* at(size_t off) const { return ws + off; }
  float* fat(size_t off) const { return reinterpret_cast<float*>(ws + off); }
  double* dat(size_t off) const { return reinterpret_cast<double*>(ws + off); }
  const float* par(int i) const { return i < 0 ? nullptr : params[i]; }
  const float* par(int op, PField f) const { return par(kG.prm[op].at[f]); }

  // op i with what its steps look at: the table row, its resources, its level and that level's extents
  struct Op { int i; const OpDesc& o; const OpRes& r; int lv; const Dims& dm; };
  Op op(int i) const { return Op{i, kOps[i], p.op[i], kG.level[kOps[i].dst], p.dims_of(kOps[i].dst)}; }

  int setup(const seunet_net_desc* desc, const float* const* prm, void* workspace, size_t bytes, hipStream_t st) {
    SEUNET_CHECK(desc && prm && workspace, "net: null argument");
    if (int e = p.init(*desc)) return e;
    SEUNET_CHECK(bytes >= p.total, "net: workspace too small (%zu < %zu bytes)", bytes, p.total);
    SEUNET_CHECK((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "net: workspace must be 256-byte aligned");
    ws = reinterpret_cast<unsigned char*>(workspace);
    params = prm;
    s = st;
    for (int i = 0; i < kNumParams; ++i)
      SEUNET_CHECK(prm[i] != nullptr || i == kG.dead, "net: parameter %s.%s is null", kG.param[i].block, kFieldName[kG.param[i].f]);
    return 0;
  }

  SrcList srcs(int i) const {
    SrcList l{};
    l.n = kG.nsrc[i];
    for (int k = 0; k < l.n; ++k) { l.ptr[k] = at(p.feat[kOps[i].src[k]]); l.C[k] = p.C[kOps[i].src[k]]; }
    return l;
  }

  // conv (+ InstanceNorm statistics) of one block: raw <- conv(src), (mean, rstd) <- stats(raw)
  int conv_and_stats(const char* nm, ConvKernel k, int taps, int dil, const SrcList& src, int cin, const float* w,
                     const float* bias, size_t wp_off, size_t raw_off, int cout, size_t mean_off, size_t rstd_off, const Dims& dm) {
    DstList dst{};
    dst.n = 1; dst.ptr[0] = at(raw_off); dst.C[0] = cout; dst.acc[0] = 0;
    mark("conv_fwd:", nm);
    if (int e = run_conv(k, p.d.dtype, taps, dil, src, cin, w, 0, at(wp_off), bias, dst, dat(p.stats), dm, s)) return e;
    if (k == ConvKernel::Naive) {   // (the naive conv leaves the statistics to a pass of their own)
      mark("stats");
      if (int e = launch_channel_stats(p.d.dtype, at(raw_off), cout, dat(p.stats), dm, s)) return e;
    }
    mark("stats");
    return launch_stats_finalize(dat(p.stats), conv_slots(k, dm, taps, dil, src.total(), cout), cout, dm.N, dm.vox(), p.d.eps, 0,
                                 fat(mean_off), fat(rstd_off), s);
  }

  // a block's epilogue, described once from its OpRes offsets for the forward and both backward passes
  GateBlock gate_block(const Op& c) const {
    return GateBlock{{at(c.r.raw), fat(c.r.mean), fat(c.r.rstd)}, c.r.cout,
                     {par(c.i, P_SE), par(c.i, P_SE2), par(c.i, P_CONV2_W), par(c.i, P_CONV2_B), p.d.negative_slope}};
  }
  CatBlock cat_block(const Op& c) const {
    const OpRes& r = c.r;
    Branch2 x{};
    if (c.o.xname && p.fuse_x) x = {Branch2::Recomputed, at(p.feat[c.o.xsrc]), fat(r.mean2), fat(r.rstd2), par(kG.prm[c.i].xw), p.d.in_channel};
    else if (c.o.xname) x = {Branch2::Stored, at(r.raw2), fat(r.mean2), fat(r.rstd2), nullptr, 0};
    return CatBlock{{at(r.raw), fat(r.mean), fat(r.rstd)}, x, r.cout, p.d.negative_slope};
  }
  // the source of a materialised x-branch conv: the padded network input
  SrcList xbranch_src(const OpDesc& o) const { return SrcList{{at(p.feat[o.xsrc])}, {8}, 1}; }
  bool skip_enc_head = false;   // inference (prediction.py:102-103 discards pred0): the encoder head and its side maps are not evaluated

  // the slice of its head (dc0_0 / dc0_1) that gated block i's two side channels feed
  struct HeadSlice { const float* w; const float* drop; int stride; float* gw; };
  HeadSlice head_slice(int i, float* const* grads = nullptr) const {
    const int h = kG.head[i], c = 2 * kG.slot[i];
    float* g = grads ? grads[kG.head_w[h]] : nullptr;
    return HeadSlice{params[kG.head_w[h]] + c, drops[h] ? drops[h] + c : nullptr, 2 * kG.sides[h], g ? g + c : nullptr};
  }

  SseHead sse_head(int i, bool first_of_level) const {
    const int h = kG.head[i];
    if (h == 0 && skip_enc_head) return SseHead{};   // (no level map: the epilogue skips the side conv altogether)
    const int acc = first_of_level ? 0 : 1;
    // general head path (classes.hip): the epilogue leaves the side map (acc: consumed by side_to_level)
    if (p.d.n_classes > 1) return SseHead{fat(p.op[i].side), nullptr, acc, nullptr, nullptr, 0};
    const HeadSlice hs = head_slice(i);
    return SseHead{nullptr, fat(p.lvl[h][kG.level[kOps[i].dst]]), acc, hs.w, hs.drop, hs.stride};
  }

  // ---- n_classes > 1 (classes.hip): a gated block's side map to and from the K level maps of its head, and the heads once per
  // (sample, class) on the [class][N][V] level maps --------------------------------------------------------------------------
  int side_to_level(const Op& c, int accumulate) {
    const HeadSlice hs = head_slice(c.i);
    return launch_side_to_level(fat(c.r.side), hs.w, hs.stride, hs.drop, hs.stride, p.d.n_classes, fat(p.lvl[kG.head[c.i]][c.lv]),
                                accumulate, c.dm, s);
  }
  // the K level-map gradients of this level folded into the gradient of the block's side map, Plan::gside (and the head-weight
  // gradient summed on the way)
  int level_to_side_grad(const Op& c, const float* g_level) {
    const HeadSlice hs = head_slice(c.i, grads);
    const int K = p.d.n_classes;
    const long long V = c.dm.vox();
    const long long cstride = c.lv == 0 ? V : (long long)c.dm.N * V, nstride = c.lv == 0 ? (long long)K * V : V;
    mark("epi_bwd:", c.o.name);
    return launch_level_to_side_grad(g_level, cstride, nstride, fat(c.r.side), hs.w, hs.stride, hs.drop, hs.stride, K,
                                     fat(p.gside), dat(p.cls_part), hs.gw, c.dm, s);
  }
  // fn(maps of (sample n, class c) on the levels l0 .. nl-1 of `maps`, n * K + c)
  template <class F> int per_sample_class(const size_t* maps, int l0, int nl, F fn) {
    const int K = p.d.n_classes, N = p.d.batch;
    for (int n = 0; n < N; ++n)
      for (int c = 0; c < K; ++c) {
        float* m[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int l = l0; l < nl; ++l) m[l] = fat(maps[l]) + ((size_t)c * N + n) * p.dims[l].vox();
        if (int e = fn(m, (size_t)n * K + c)) return e;
      }
    return 0;
  }

  // every conv weight of a pass repacked into its MFMA layout by one launch per kernel (the parameters change every step)
  int pack_all_weights(bool dgrad) {
    if (p.d.conv_impl == SEUNET_CONV_NAIVE) return 0;
    mark("pack_w");
    std::vector<ConvPackJob> jobs;
    // PyTorch weight w (cout, cin, k,k,k), read transposed / mirrored by the data gradient; src_c -> dst_c: the channels of the
    // conv's source and destination tensors
    auto add = [&](ConvKernel k, const float* w, size_t wp, int taps, int cin, int cout, int src_c, int dst_c) {
      jobs.push_back({k, w, at(wp), taps, cin, cout, dgrad ? 1 : 0, src_c, dst_c});
    };
    for (int i = 0; i < kNumOps; ++i) {
      const OpDesc& o = kOps[i];
      if (!is_conv(o)) continue;
      const OpRes& r = p.op[i];
      const int ctot = srcs(i).total();
      if (!dgrad) {
        add(r.fwd, par(i, P_CONV1_W), r.wp_f, r.taps, r.cin, r.cout, ctot, r.cout);
        if (o.xname && !p.fuse_x) add(r.x_fwd, par(kG.prm[i].xw), r.wp_x, 1, p.d.in_channel, r.cout, 8, r.cout);
      } else if (r.need_dgrad) {
        add(r.dgrad, par(i, P_CONV1_W), r.wp_d, r.taps, r.cin, r.cout, r.cout, ctot);
      }
    }
    return launch_conv_pack(p.d.dtype, jobs.data(), (int)jobs.size(), s);
  }

  // ---- forward: one step per op kind --------------------------------------------------------------------------------------
  bool lvl_written[2][4] = {};   // a head's level map has its first block's contribution: the next one adds

  int gated_forward(const Op& c) {
    const int h = kG.head[c.i];
    if (int e = conv_and_stats(c.o.name, c.r.fwd, 27, c.o.dil, srcs(c.i), c.r.cin, par(c.i, P_CONV1_W), par(c.i, P_CONV1_B), c.r.wp_f,
                               c.r.raw, c.r.cout, c.r.mean, c.r.rstd, c.dm)) return e;
    const SseHead hd = sse_head(c.i, !lvl_written[h][c.lv]);
    lvl_written[h][c.lv] = true;
    mark("epi_fwd:", c.o.name);
    if (int e = launch_sse_fwd(p.d.dtype, gate_block(c), at(p.feat[c.o.dst]), hd, c.dm, s)) return e;
    return hd.side_out ? side_to_level(c, hd.level_accumulate) : 0;
  }

  int cat_forward(const Op& c) {
    const OpRes& r = c.r;
    const CatBlock blk = cat_block(c);
    if (int e = conv_and_stats(c.o.name, r.fwd, 1, 1, srcs(c.i), r.cin, par(c.i, P_CONV1_W), nullptr, r.wp_f, r.raw, r.cout, r.mean,
                               r.rstd, c.dm)) return e;
    PoolOut pool_out{};
    if (blk.b.kind == Branch2::Recomputed) {
      // x-branch: statistics from the input's moments, values recomputed inside the epilogue (never stored)
      mark("stats");
      if (int e = launch_xbranch_moments(p.d.dtype, blk.b.src, dat(p.xmom), c.dm, s)) return e;
      if (int e = launch_xbranch_stats(dat(p.xmom), xbranch_moment_slots(c.dm), blk.b.w2, r.cout, p.d.in_channel, c.dm.N, c.dm.vox(),
                                       p.d.eps, fat(r.mean2), fat(r.rstd2), dat(r.xtot), s)) return e;
      // the max-pool that consumes this block (ec33 -> pool0, ec63 -> pool1, ec93 -> pool2) is written by the same kernel,
      // with the position of each maximum for the backward pass
      SEUNET_CHECK(r.fused >= 0, "net: internal: %s has no max-pool to write", c.o.name);
      pool_out = PoolOut{at(p.feat[kOps[r.fused].dst]), reinterpret_cast<unsigned*>(at(p.op[r.fused].pool_idx))};
    } else if (blk.b.kind == Branch2::Stored) {
      if (int e = conv_and_stats(c.o.xname, r.x_fwd, 1, 1, xbranch_src(c.o), p.d.in_channel, par(kG.prm[c.i].xw), nullptr, r.wp_x, r.raw2,
                                 r.cout, r.mean2, r.rstd2, c.dm)) return e;
    }
    mark("cat_fwd:", c.o.name);
    return launch_cat_fwd(p.d.dtype, blk, at(p.feat[c.o.dst]), pool_out, c.dm, s);
  }

  int pool_forward(const Op& c) {
    if (c.r.fused >= 0) return 0;          // written by its aggregation block's epilogue
    const int t = c.o.src[0];
    mark("pool_fwd:", c.o.name);
    return launch_maxpool_fwd(p.d.dtype, at(p.feat[t]), p.C[t], at(p.feat[c.o.dst]), p.dims_of(t), s);
  }

  int up_forward(const Op& c) {
    const int t = c.o.src[0];
    mark("up_fwd:", c.o.name);
    return launch_upsample2_fwd(p.d.dtype, at(p.feat[t]), p.C[t], at(p.feat[c.o.dst]), p.dims_of(t), s);
  }

  // the encoder head (4 levels; skipped when pred0 is null) and the decoder head (3): logits (N, K, D, H, W)
  int heads_forward(float* pred0, float* pred1) {
    float* const pred[2] = {pred0, pred1};
    const Dims d1{1, p.dims[0].D, p.dims[0].H, p.dims[0].W};
    mark("head_fwd");
    for (int h = 0; h < 2; ++h) {
      if (pred[h] == nullptr) continue;
      const int nl = 4 - h;
      if (p.d.n_classes > 1) {
        if (int e = per_sample_class(p.lvl[h], 0, nl, [&](float* const* lm, size_t nc) {
              return launch_head_fwd(lm, nl, par(kG.head_b[h]) + nc % p.d.n_classes, pred[h] + nc * d1.vox(), d1, s);
            })) return e;
      } else {
        const float* lm[4] = {fat(p.lvl[h][0]), fat(p.lvl[h][1]), fat(p.lvl[h][2]), fat(p.lvl[h][3])};
        if (int e = launch_head_fwd(lm, nl, par(kG.head_b[h]), pred[h], p.dims[0], s)) return e;
      }
    }
    mark("outside");
    return 0;
  }

  int forward(const float* x, const float* drop1, const float* drop2, float* pred0, float* pred1) {
    skip_enc_head = pred0 == nullptr;
    drops[0] = drop1; drops[1] = drop2;
    if (int e = pack_all_weights(false)) return e;
    mark("pack_input");
    if (int e = launch_pack_input(p.d.dtype, x, p.d.in_channel, at(p.feat[T_X0]), p.dims[0], s)) return e;
    for (int i = 0; i < kNumOps; ++i) {
      const Op c = op(i);
      const OpKind k = c.o.kind;
      if (int e = k == OP_GATED ? gated_forward(c) : k == OP_CAT ? cat_forward(c) : k == OP_POOL ? pool_forward(c) : up_forward(c))
        return e;
    }
    return heads_forward(pred0, pred1);
  }

  // ---- backward: one step per op kind, in reverse walk order ----------------------------------------------------------------
  const float* g_pred[2] = {nullptr, nullptr};   // the logit gradients of the two heads
  float* const* grads = nullptr;                 // parameter gradients in registry order (null = not asked for)
  bool written[T_COUNT] = {};                    // grad[t] holds a gradient: the next one adds
  std::vector<float*> zero_ptrs;                 // gradients that are identically zero, cleared by one launch after the walk
  std::vector<int> zero_counts;
  hipEvent_t decoder_done = nullptr;   // recorded once every gradient of the decoder blocks (dc1 .. dc6, dc22, dc42) is final

  float* gpar(int op, PField f) const { const int k = kG.prm[op].at[f]; return k < 0 ? nullptr : grads[k]; }

  // The slab reduction of the last weight gradient, not yet launched (wgrad.h).  Nothing reads a weight gradient inside the
  // walk, so the reduction need not sit between wgrad(L) and dgrad(L): it rides the next finalize launch of the walk
  // (take_pending: gated_backward, cat_backward; the last one rides the zeroing launch after the walk) as extra workgroups.
  // It has to run before the next weight gradient overwrites wgrad_ws and before decoder_done is recorded: flush_pending.
  WgReduceJob pending;
  WgReduceJob* defer() { return g_wgrad_defer ? &pending : nullptr; }
  WgReduceJob take_pending() { const WgReduceJob j = pending; pending = WgReduceJob{}; return j; }
  int flush_pending() {
    if (pending.blocks() == 0) return 0;
    mark("wgrad:flush");
    return launch_wgrad_reduce(take_pending(), s);
  }
  // one weight gradient of the walk into the shared workspace
  int walk_wgrad(ConvKernel k, int taps, int dil, const SrcList& x, int cin, const void* dy, int cout, float* gw, const Dims& dm) {
    if (int e = flush_pending()) return e;   // (only a second weight gradient of one op finds one: the materialised x-branch's)
    return run_wgrad(k, p.d.dtype, taps, dil, x, cin, dy, cout, gw, at(p.wgrad_ws), p.wgrad_ws_bytes, dm, s, defer());
  }

  // gradient w.r.t. the raw conv output is in grad[dst]; produce weight gradient and input gradients
  int conv_backward(const Op& c) {
    const OpDesc& o = c.o;
    const OpRes& r = c.r;
    const SrcList x = srcs(c.i);
    if (float* gw = gpar(c.i, P_CONV1_W)) {
      mark("wgrad:", o.name);
      if (int e = walk_wgrad(r.wgrad, r.taps, o.dil, x, r.cin, at(p.grad[o.dst]), r.cout, gw, c.dm)) return e;
    }
    if (!r.need_dgrad) return 0;
    const SrcList gsrc{{at(p.grad[o.dst])}, {r.cout}, 1};
    DstList gd{};
    gd.n = x.n;
    for (int k = 0; k < x.n; ++k) {
      const int t = o.src[k];
      gd.C[k] = p.C[t];
      gd.ptr[k] = is_input(t) ? nullptr : at(p.grad[t]);
      gd.acc[k] = (!is_input(t) && written[t]) ? 1 : 0;
      if (!is_input(t)) written[t] = true;
    }
    mark("dgrad:", o.name);
    return run_conv(r.dgrad, p.d.dtype, r.taps, o.dil, gsrc, r.cout, par(c.i, P_CONV1_W), 1, at(r.wp_d), nullptr, gd, nullptr, c.dm, s);
  }

  // heads: level gradients = transposed interpolation of the logit gradients
  int heads_backward() {
    const Dims d1{1, p.dims[0].D, p.dims[0].H, p.dims[0].W};
    mark("head_bwd");
    for (int h = 0; h < 2; ++h) {
      const int nl = 4 - h;
      float* gb = grads[kG.head_b[h]];
      if (p.d.n_classes > 1) {     // the bias gradient of a class = its per-sample sums added up
        if (int e = per_sample_class(p.glvl[h], 1, nl, [&](float* const* gl, size_t nc) {
              return launch_head_bwd(g_pred[h] + nc * d1.vox(), gl, nl, fat(p.head_tmp), fat(p.cls_bias) + nc, d1, s);
            })) return e;
        if (gb)
          if (int e = launch_class_bias_grad(fat(p.cls_bias), p.d.batch, p.d.n_classes, gb, s)) return e;
      } else {
        float* gl[4] = {nullptr, fat(p.glvl[h][1]), fat(p.glvl[h][2]), nl == 4 ? fat(p.glvl[h][3]) : nullptr};
        if (int e = launch_head_bwd(g_pred[h], gl, nl, fat(p.head_tmp), gb, p.dims[0], s)) return e;
      }
    }
    return 0;
  }

  int gated_backward(const Op& c) {
    const OpDesc& o = c.o;
    const int h = kG.head[c.i], P_slots = epi_partials(c.dm);
    const GateBlock blk = gate_block(c);
    SseBwdIn g{written[o.dst] ? at(p.grad[o.dst]) : nullptr, nullptr, c.lv == 0 ? g_pred[h] : fat(p.glvl[h][c.lv])};
    SseHead hd = sse_head(c.i, false);
    float* g_head = head_slice(c.i, grads).gw;
    if (p.d.n_classes > 1) {   // general head path: the block's passes take the side map's gradient
      if (int e = level_to_side_grad(c, g.g_level)) return e;
      g.g_level = nullptr;
      g.g_side = fat(p.gside);
      hd.side_out = nullptr;
      g_head = nullptr;          // (written above; the finalize kernel must not overwrite it)
    }
    mark("epi_bwd:", o.name);   // pass A: f64 sums + parameter-gradient records
    if (int e = launch_sse_bwd_sums(p.d.dtype, blk, g, hd, SseSums{dat(p.stats), fat(p.pgrad)}, c.dm, s)) return e;
    mark("stats");
    const WgReduceJob rider = take_pending();
    if (int e = launch_gate_bwd_finalize(dat(p.stats), P_slots, c.r.cout, c.dm.N, c.dm.vox(), fat(p.m1), fat(p.m2), fat(p.pgrad),
                                         c.dm.N * P_slots, gpar(c.i, P_SE), gpar(c.i, P_SE2), gpar(c.i, P_CONV2_W),
                                         gpar(c.i, P_CONV2_B), g_head, s, &rider)) return e;
    mark("in_bwd:", o.name);    // pass B: recompute dxhat, apply the InstanceNorm backward, store draw over g_e
    if (int e = launch_sse_bwd_apply(p.d.dtype, blk, g, hd, SseApply{fat(p.m1), fat(p.m2), at(p.grad[o.dst])}, c.dm, s)) return e;
    written[o.dst] = true;
    // conv1.bias feeds an affine-less InstanceNorm: its gradient is identically zero; zeroed in one
    // launch after the walk
    if (float* gb = gpar(c.i, P_CONV1_B)) { zero_ptrs.push_back(gb); zero_counts.push_back(c.r.cout); }
    return conv_backward(c);
  }

  int cat_backward(const Op& c) {
    const OpDesc& o = c.o;
    const OpRes& r = c.r;
    const int P_slots = epi_partials(c.dm);
    SEUNET_CHECK(written[o.dst], "net: internal: gradient of %s output missing", o.name);
    const CatBlock blk = cat_block(c);
    const bool two = blk.b.kind != Branch2::None, recomputed = blk.b.kind == Branch2::Recomputed;
    float* gxw = two ? grads[kG.prm[c.i].xw] : nullptr;   // the x-branch weight's gradient, if asked for
    const void* g_out = at(p.grad[o.dst]);
    // a fused max-pool's gradient is added on the fly by both passes -- no read-modify-write of the full-resolution gradient
    PoolGrad pool{};
    if (r.fused >= 0) pool = PoolGrad{reinterpret_cast<const unsigned*>(at(p.op[r.fused].pool_idx)), at(p.grad[kOps[r.fused].dst])};
    mark("cat_bwd:", o.name);   // pass A; a recomputed x-branch also sums what its weight gradient is formed from
    const CatSums sums{dat(p.stats), dat(p.stats2), recomputed && gxw ? dat(p.xwp) : nullptr};
    if (int e = launch_cat_bwd_sums(p.d.dtype, blk, g_out, pool, sums, c.dm, s)) return e;
    mark("stats");   // one launch: both branches' means, the recomputed x-branch's weight gradient, the pending slab reduction
    const CatXwFinalize xwf{dat(p.xwp), dat(r.xtot), blk.b.w2, p.d.in_channel, p.d.eps, recomputed ? gxw : nullptr};
    const WgReduceJob rider = take_pending();
    if (int e = launch_cat_bwd_finalize(dat(p.stats), two ? dat(p.stats2) : nullptr, P_slots, r.cout, c.dm.N, c.dm.vox(), fat(p.m1),
                                        fat(p.m2), fat(p.m1b), fat(p.m2b), xwf, s, &rider)) return e;
    // pass B: draw over g_out; a stored x-branch's draw goes to gx, a recomputed one adds its input-gradient term on the fly
    mark("in_bwd:", o.name);
    CatApply ap{fat(p.m1), fat(p.m2), fat(p.m1b), fat(p.m2b), at(p.grad[o.dst]), two && !recomputed ? at(p.gx) : nullptr, nullptr, 0};
    if (recomputed && grad_x) { ap.gx_out = gxl(c.lv); ap.gx_acc = c.lv == 1 ? 1 : 0; }
    if (int e = launch_cat_bwd_apply(p.d.dtype, blk, g_out, pool, ap, c.dm, s)) return e;
    if (two && !recomputed) {
      if (grad_x) {   // gx_l (+)= W_x^T d2 from the stored d2 (level 1: on top of unpool_1(gx_2))
        mark("input_grad:", o.xname);
        if (int e = launch_xgrad_contract(p.d.dtype, at(p.gx), r.cout, par(kG.prm[c.i].xw), p.d.in_channel, gxl(c.lv), c.lv == 1 ? 1 : 0, c.dm, s)) return e;
      }
      if (gxw) {
        mark("wgrad:", o.xname);
        if (int e = walk_wgrad(r.x_wgrad, 1, 1, xbranch_src(o), p.d.in_channel, at(p.gx), r.cout, gxw, c.dm)) return e;
      }
    }
    return conv_backward(c);
  }

  int pool_backward(const Op& c) {
    const OpDesc& o = c.o;
    const int t = o.src[0];
    if (grad_x && o.dst == T_X2) {
      // pool1x: gx_1 = unpool_1(gx_2), arg-max of the stored X1 (ec63's pass B then adds its own term)
      mark("input_grad:unpool1");
      if (int e = launch_xgrad_unpool(p.d.dtype, at(p.feat[T_X1]), p.d.in_channel, gxl(2), gxl(1), p.dims[1], s)) return e;
    }
    if (is_input(t)) return 0;
    SEUNET_CHECK(written[o.dst], "net: internal: gradient of %s output missing", o.name);
    mark("pool_bwd:", o.name);
    if (c.r.fused >= 0) {
      // nothing to launch: the aggregation block that produced tensor t adds this gradient in both of its backward passes
      // (dc5, dc3 and dc1 have already differentiated E1, E3 and E5, the tensors these pools read)
      SEUNET_CHECK(written[t], "net: internal: gradient of %s input missing before its deferred pool gradient", o.name);
      return 0;
    }
    if (int e = launch_maxpool_bwd(p.d.dtype, at(p.feat[t]), at(p.grad[o.dst]), p.C[t], at(p.grad[t]), written[t] ? 1 : 0,
                                   p.dims_of(t), s)) return e;
    written[t] = true;
    return 0;
  }

  int up_backward(const Op& c) {
    const int t = c.o.src[0];
    SEUNET_CHECK(written[c.o.dst], "net: internal: gradient of %s output missing", c.o.name);
    mark("up_bwd:", c.o.name);
    if (int e = launch_upsample2_bwd(p.d.dtype, at(p.grad[c.o.dst]), p.C[t], at(p.grad[t]), written[t] ? 1 : 0, p.dims_of(t), s)) return e;
    written[t] = true;
    return 0;
  }

  int backward(const float* g_pred0, const float* g_pred1, const float* drop1, const float* drop2, float* const* grads_) {
    drops[0] = drop1; drops[1] = drop2;
    g_pred[0] = g_pred0; g_pred[1] = g_pred1;
    grads = grads_;
    if (int e = pack_all_weights(true)) return e;
    if (int e = heads_backward()) return e;
    for (int i = kNumOps - 1; i >= 0; --i) {
      if (decoder_done && i == kG.first_up) {
        // the walk is in reverse forward order: everything after up0 (the decoder) has been differentiated.  Its parameter
        // gradients are final from here on (the heads' weights are not: the encoder blocks still add to dc0_0)
        if (int e = flush_pending()) return e;
        SEUNET_HIP(hipEventRecord(decoder_done, s));
      }
      const Op c = op(i);
      const OpKind k = c.o.kind;
      if (int e = k == OP_GATED ? gated_backward(c) : k == OP_CAT ? cat_backward(c) : k == OP_POOL ? pool_backward(c) : up_backward(c))
        return e;
    }
    if (!zero_ptrs.empty() || pending.blocks() > 0) {   // with the last weight gradient's slab reduction as its rider
      mark("stats");
      const WgReduceJob rider = take_pending();
      if (int e = launch_multi_zero(zero_ptrs.data(), zero_counts.data(), (int)zero_ptrs.size(), s, &rider)) return e;
    }
    if (grad_x) {
      // grad_x = convT_ec1(draw_ec1) + gx_0 + unpool_0(gx_1); ec1's pass B left draw_ec1 in grad[T_E0]
      mark("input_grad:ec1");
      if (int e = launch_input_grad(p.d.dtype, at(p.grad[T_E0]), p.C[T_E0], par(0, P_CONV1_W), at(p.feat[T_X0]), p.d.in_channel,
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
  return desc ? kNumParams : -1;
}

int seunet_net_param_info(const seunet_net_desc* desc, int index, char* name, int name_cap, int* shape5, int* ndim) {
  SEUNET_CHECK(desc && name && shape5 && ndim, "param_info: null argument");
  SEUNET_CHECK(index >= 0 && index < kNumParams, "param_info: index %d out of range", index);
  const seunet_net_desc& d = *desc;
  const ParamDesc& q = kG.param[index];
  snprintf(name, (size_t)name_cap, "%s.%s", q.block, kFieldName[q.f]);
  const int ci = q.cin ? q.cin * d.width_mult : d.in_channel, co = q.cout * d.width_mult;
  const int shapes[][5] = {{co, ci, q.k, q.k, q.k}, {co}, {2, co, 1, 1, 1}, {2}, {1, co, 1, 1, 1}, {1, co, 1, 1, 1},
                           {d.n_classes, q.cin, 1, 1, 1}, {d.n_classes}};   // by PField; a vector's trailing extents are 0
  for (int k = 0; k < 5; ++k) shape5[k] = shapes[q.f][k];
  *ndim = shapes[q.f][1] ? 5 : 1;
  return 0;
}

size_t seunet_net_workspace_bytes(const seunet_net_desc* desc) {
  Plan p;
  return desc && p.init(*desc) == 0 ? p.total : 0;
}

// Diagnostic (host only, not in the public header): buffer `index` of the plan in the order it was taken -- its name, offset and
// bytes before alignment padding; the workspace's buffers first, then the separate input-gradient scratch's under "ig:" names.
// 0, or non-zero for a bad descriptor or an index past the end.  tests/test_net_layout_host.py pins the layout with it.
int seunet_debug_net_layout(const seunet_net_desc* desc, int index, char* name, int cap, size_t* offset, size_t* bytes) {
  SEUNET_CHECK(desc && name && offset && bytes, "debug_net_layout: null argument");
  Plan p;
  if (int e = p.init(*desc)) return e;
  if (index < 0 || index >= (int)p.log.size()) return 1;
  const Take& t = p.log[index];
  snprintf(name, (size_t)cap, "%s%s%s", t.what, t.of[0] ? ":" : "", t.of);
  *offset = t.off;
  *bytes = t.bytes;
  return 0;
}

// Diagnostic (process-global, not in the public header): on (the default) = the backward walk defers each weight gradient's
// slab reduction into the next finalize launch; off = every weight gradient reduces at once, in a launch of its own.  The two
// give the same bits (tests/test_wgrad_deferred_gpu.py).  Returns the previous setting.
int seunet_debug_net_wgrad_defer(int on) {
  const int was = g_wgrad_defer ? 1 : 0;
  g_wgrad_defer = on != 0;
  return was;
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
  int i;
  bool xbranch;
  if (int e = plan_and_find(*desc, -1, name, &p, &i, &xbranch)) return e;
  SEUNET_CHECK(workspace_bytes >= p.total, "net_read_tensor: workspace too small");
  SEUNET_CHECK(i >= 0, "net_read_tensor: no block named %s", name);
  const unsigned char* ws = reinterpret_cast<const unsigned char*>(workspace);
  const OpDesc& o = kOps[i];
  const OpRes& r = p.op[i];
  const Dims& dm = p.dims_of(o.dst);
  const size_t raw = xbranch ? r.raw2 : r.raw, mean = xbranch ? r.mean2 : r.mean, rstd = xbranch ? r.rstd2 : r.rstd;
  // (an x-branch is the raw-input branch of an aggregation block; materialised when in_channel > 2)
  SEUNET_CHECK(!xbranch || (which >= 0 && which <= 2), "net_read_tensor: which=%d is not stored for an x-branch", which);
  if (channels) *channels = which == 3 ? p.C[o.dst] : r.cout;
  if (xbranch && which == 0 && p.fuse_x) {
    // in_channel <= 2: the branch is recomputed inside the aggregation epilogue and leaves no tensor: recompute it here by the
    // same device function, from the packed input in the workspace and the caller's weights
    SEUNET_CHECK(params != nullptr, "net_read_tensor: the recomputed x-branch %s needs the parameter list", name);
    const float* w = params[kG.prm[i].xw];
    SEUNET_CHECK(w, "net_read_tensor: no weight for %s", name);
    return launch_xbranch_values(p.d.dtype, ws + p.feat[o.xsrc], w, r.cout, p.d.in_channel, out, dm, (hipStream_t)s);
  }
  if (which == 0) return launch_unpack_cl(p.d.dtype, ws + raw, r.cout, out, dm, (hipStream_t)s);
  if (which == 3) return launch_unpack_cl(p.d.dtype, ws + p.feat[o.dst], p.C[o.dst], out, dm, (hipStream_t)s);
  SEUNET_CHECK(which == 1 || which == 2, "net_read_tensor: which=%d", which);
  SEUNET_HIP(hipMemcpyAsync(out, ws + (which == 1 ? mean : rstd), (size_t)p.d.batch * r.cout * 4, hipMemcpyDeviceToDevice, (hipStream_t)s));
  return 0;
}

static_assert((int)ConvKernel::Naive == SEUNET_KERNEL_NAIVE && (int)ConvKernel::Tiled == SEUNET_KERNEL_TILED &&
                  (int)ConvKernel::Stream == SEUNET_KERNEL_STREAM && (int)ConvKernel::March == SEUNET_KERNEL_MARCH &&
                  (int)ConvKernel::Wgrad1x1 == SEUNET_KERNEL_WGRAD1X1,
              "SEUNET_KERNEL_* are the values of ConvKernel");

int seunet_net_conv_info(const seunet_net_desc* desc, int index, seunet_conv_info* out) {
  SEUNET_CHECK(desc && out, "net_conv_info: null argument");
  Plan p;
  int i;
  if (int e = plan_and_find(*desc, index, nullptr, &p, &i)) return e;
  SEUNET_CHECK(index >= 0, "net_conv_info: index %d out of range", index);
  SEUNET_CHECK(i >= 0, "net_conv_info: index %d is past the last convolution (%d)", index, kG.nconv);
  const OpDesc& o = kOps[i];
  const OpRes& r = p.op[i];
  const Dims& dm = p.dims_of(o.dst);
  *out = seunet_conv_info{};
  snprintf(out->name, sizeof out->name, "%s", o.name);
  out->taps = r.taps;
  out->dilation = o.kind == OP_GATED ? o.dil : 1;
  out->level = kG.level[o.dst];
  out->dims = seunet_dims{dm.N, dm.D, dm.H, dm.W};
  out->nsrc = kG.nsrc[i];
  for (int k = 0; k < out->nsrc; ++k) { out->src_c[k] = p.C[o.src[k]]; out->src_is_input[k] = is_input(o.src[k]) ? 1 : 0; }
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
  out->src_dist = p.src_dist(i);
  return 0;
}

size_t seunet_net_input_grad_bytes(const seunet_net_desc* desc) {
  if (!desc) { (void)fail("net_input_grad_bytes: null descriptor"); return 0; }
  Plan p;
  return p.init(*desc) == 0 ? p.ig_total : 0;
}

// the one body of the three backward entry points; grad_x null: no input gradient, `scratch` is not looked at
int seunet_net_backward_input(const seunet_net_desc* desc, const float* const* params, const float* g_pred0, const float* g_pred1,
                              const float* drop1, const float* drop2, float* const* grads, float* grad_x, void* scratch,
                              size_t scratch_bytes, void* workspace, size_t workspace_bytes, seunet_stream_t s,
                              void* decoder_done_event) {
  if (grad_x) SEUNET_CHECK(g_pred0 && g_pred1 && grads && scratch, "net_backward_input: null tensor");
  SEUNET_CHECK(g_pred0 && g_pred1 && grads, "net_backward: null tensor");
  Exec ex;
  if (int e = ex.setup(desc, params, workspace, workspace_bytes, (hipStream_t)s)) return e;
  if (grad_x) {
    SEUNET_CHECK(scratch_bytes >= ex.p.ig_total, "net_backward_input: scratch too small (%zu < %zu bytes)", scratch_bytes, ex.p.ig_total);
    SEUNET_CHECK((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "net_backward_input: scratch must be 256-byte aligned");
    ex.grad_x = grad_x;
    ex.igs = reinterpret_cast<unsigned char*>(scratch);
  }
  ex.decoder_done = reinterpret_cast<hipEvent_t>(decoder_done_event);
  return ex.backward(g_pred0, g_pred1, drop1, drop2, grads);
}

int seunet_net_backward_ev(const seunet_net_desc* desc, const float* const* params, const float* g_pred0,
                           const float* g_pred1, const float* drop1, const float* drop2, float* const* grads,
                           void* workspace, size_t workspace_bytes, seunet_stream_t s, void* decoder_done_event) {
  return seunet_net_backward_input(desc, params, g_pred0, g_pred1, drop1, drop2, grads, nullptr, nullptr, 0, workspace,
                                   workspace_bytes, s, decoder_done_event);
}

int seunet_net_backward(const seunet_net_desc* desc, const float* const* params, const float* g_pred0,
                        const float* g_pred1, const float* drop1, const float* drop2, float* const* grads,
                        void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  return seunet_net_backward_ev(desc, params, g_pred0, g_pred1, drop1, drop2, grads, workspace, workspace_bytes, s, nullptr);
}

}  // extern "C"
