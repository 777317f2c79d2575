// extern "C" entry points of libseunet_hip.so (per-op part; the whole-network calls live in net.cpp).
// Thin argument marshalling only: every function validates, forwards to a launcher -- the convolutions and weight gradients
// to their family's dispatch by kernel (conv.h run_conv / launch_conv_pack, wgrad.h run_wgrad) -- and returns a status.
#include "seunet_common.h"
#include "epilogue.h"
#include "volume.h"
#include "wgrad.h"
#include "../../include/seunet_hip.h"

using namespace seunet;

static inline Dims D(seunet_dims d) { return Dims{d.n, d.d, d.h, d.w}; }
static inline hipStream_t S(seunet_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// the lists of a conv call; without pointers (channels_only, dst null) the form a *_supported query takes
static int make_src(int nsrc, const void* const* src, const int* src_c, SrcList& l, bool channels_only = false) {
  SEUNET_CHECK(nsrc >= 1 && nsrc <= 3 && (src || channels_only) && src_c, "bad source list");
  l = SrcList{};
  l.n = nsrc;
  for (int i = 0; i < nsrc; ++i) { l.ptr[i] = src ? src[i] : nullptr; l.C[i] = src_c[i]; }
  return 0;
}
static int make_dst(int ndst, void* const* dst, const int* dst_c, const int* dst_acc, DstList& dl) {
  SEUNET_CHECK(ndst >= 1 && ndst <= 3 && dst_c, "bad destination list");
  dl = DstList{};
  dl.n = ndst;
  for (int i = 0; i < ndst; ++i) { dl.ptr[i] = dst ? dst[i] : nullptr; dl.C[i] = dst_c[i]; dl.acc[i] = dst_acc ? dst_acc[i] : 0; }
  return 0;
}

namespace seunet { extern unsigned long long* g_conv_debug; }

extern "C" {

// diagnostic hook (not part of the public header): device buffer of 8 u64 that -DSEUNET_STAMP builds add cycle sums to
int seunet_debug_set_buffer(void* p) { seunet::g_conv_debug = reinterpret_cast<unsigned long long*>(p); return 0; }
// diagnostic hook (not part of the public header, host only): the kernel form an x2 up-sampling pass takes for these
// arguments -- 0 gather, 1 tiled, 2 march
int seunet_debug_upsample2_form(int dtype, int c, seunet_dims dims, int backward) { return upsample2_form(dtype, c, D(dims), backward != 0); }

// diagnostic hook (not part of the public header, host only): the workspace layout of a volume operation as its launcher
// carves it.  op: 0 cc, 1 get_l, 2 edt, 3 lib_weight, 4 break_weight, 5 skeleton_branches, 6 dti, 7 skeleton, 8 parse_assign,
// 9 binary_morph, 10 mesh, 11 mesh_label, 12 edt_sampling, 13 surface (count), 14 surface_emit (extents of the box), 15 label,
// 16 euler, 17 betti (the last two for the whole volume: one tile), 18 cross_section.
// Returns the number of sub-buffers (0: extents the op rejects, -1: no such op) and writes (offset, bytes up to the next
// sub-buffer or the end) of the first `cap`.
int seunet_debug_volume_layout(int op, int n0, int n1, int n2, size_t* offsets, int cap) {
  if (n0 < 1 || n1 < 1 || n2 < 1) return 0;
  size_t at[16];                       // no operation has more than 14 sub-buffers
  WsCarver c(nullptr);
  c.log = at;
  c.log_cap = 16;
  switch (op) {
    case 0: cc_ws(c, n0, n1, n2); break;
    case 1: get_l_ws(c, n0, n1, n2); break;
    case 2: case 8: edt_ws(c, n0, n1, n2); break;
    case 3: lib_weight_ws(c, n0, n1, n2); break;
    case 4: break_weight_ws(c, n0, n1, n2); break;
    case 5: branches_ws(c, n0, n1, n2); break;
    case 6: dti_ws(c, n0, n1, n2); break;
    case 7: if (!skeleton_ws(c, n0, n1, n2)) return 0; break;
    case 9: morph_ws(c, n0, n1, n2); break;
    case 10: if ((long long)n0 * n1 * n2 >= (1ll << 31)) return 0; mesh_ws(c, n0, n1, n2); break;
    case 11: if ((long long)n0 * n1 * n2 >= (1ll << 31)) return 0; mesh_label_ws(c, n0, n1, n2); break;
    case 12: edt_sampling_ws(c, n0, n1, n2); break;
    case 13: if ((long long)n0 * n1 * n2 >= (1ll << 31)) return 0; surface_ws(c, n0, n1, n2); break;
    case 14: if ((long long)n0 * n1 * n2 >= (1ll << 31)) return 0; surface_emit_ws(c, n0, n1, n2); break;
    case 15: if ((long long)n0 * n1 * n2 >= (1ll << 31)) return 0; label_ws(c, n0, n1, n2); break;
    case 16: if ((long long)n0 * n1 * n2 >= (1ll << 31)) return 0; euler_ws(c, n0, n1, n2, 1); break;
    case 17: if ((long long)n0 * n1 * n2 >= (1ll << 31)) return 0; betti_ws(c, n0, n1, n2, 1); break;
    case 18: if ((long long)n0 * n1 * n2 >= (1ll << 31)) return 0; cross_section_ws(c, n0, n1, n2); break;
    default: return -1;
  }
  if (c.taken > c.log_cap) return -1;
  for (int i = 0; i < c.taken && i < cap && offsets; ++i) {
    offsets[2 * i] = at[i];
    offsets[2 * i + 1] = (i + 1 < c.taken ? at[i + 1] : c.bytes()) - at[i];
  }
  return c.taken;
}

int seunet_version(void) { return 201; }
const char* seunet_last_error(void) { return get_error(); }

int seunet_init(int device) {
  int count = 0, prev = 0;
  SEUNET_HIP(hipGetDeviceCount(&count));
  SEUNET_CHECK(device >= 0 && device < count, "init: device %d out of range (%d visible)", device, count);
  SEUNET_HIP(hipGetDevice(&prev));
  SEUNET_HIP(hipSetDevice(device));
  const void* page = seunet::device_zero_page();
  (void)hipSetDevice(prev);
  SEUNET_CHECK(page != nullptr, "init: could not allocate the zero page on device %d", device);
  return 0;
}

int seunet_pack_cl(int dtype, const float* in, int c, void* out, int c_pad, seunet_dims dims, seunet_stream_t s) {
  SEUNET_CHECK(in && out, "pack_cl: null tensor");
  return launch_pack_cl(dtype, in, c, out, c_pad, D(dims), S(s));
}
int seunet_unpack_cl(int dtype, const void* in, int c, float* out, seunet_dims dims, seunet_stream_t s) {
  SEUNET_CHECK(in && out, "unpack_cl: null tensor");
  return launch_unpack_cl(dtype, in, c, out, D(dims), S(s));
}

// the forward convs: validate, build the lists, run on the kernel the entry point names (conv.h)
static inline ConvKernel fwd_kernel(int impl) { return impl == SEUNET_CONV_NAIVE ? ConvKernel::Naive : ConvKernel::Tiled; }
// one weight packed for kernel k: a list of one job
static int pack_one(ConvKernel k, int dtype, const float* w, int taps, int cin_w, int cout_w, int tflip, int src_c, int dst_c,
                    void* wpack, seunet_stream_t s) {
  const ConvPackJob j{k, w, wpack, taps, cin_w, cout_w, tflip, src_c, dst_c};
  return launch_conv_pack(dtype, &j, 1, S(s));
}
size_t seunet_conv_wpack_bytes(int dtype, int taps, int cin, int cout) { return conv_igemm_wpack_bytes(dtype, taps, cin, cout); }
int seunet_conv_pack_weights(int dtype, const float* w, int taps, int cin, int cout, int tflip, void* wpack, seunet_stream_t s) {
  SEUNET_CHECK(w && wpack, "conv_pack_weights: null tensor");
  return pack_one(ConvKernel::Tiled, dtype, w, taps, cin, cout, tflip, 0, 0, wpack, s);
}
int seunet_conv_stats_slots(int impl, int taps, int dilation, seunet_dims dims) {
  return conv_slots(fwd_kernel(impl), D(dims), taps, dilation, 0, 0);
}
int seunet_conv3d_fwd(int dtype, int impl, int taps, int dilation, int nsrc, const void* const* src, const int* src_c, int cin,
                      const void* weights, int tflip, const float* bias, int ndst, void* const* dst, const int* dst_c,
                      const int* dst_acc, double* stats_partial, seunet_dims dims, seunet_stream_t s) {
  SrcList sl; DstList dl;
  if (int e = make_src(nsrc, src, src_c, sl)) return e;
  SEUNET_CHECK(ndst >= 1 && ndst <= 3 && dst && dst_c && weights, "conv3d_fwd: bad destination list / weights");
  if (int e = make_dst(ndst, dst, dst_c, dst_acc, dl)) return e;
  const ConvKernel k = fwd_kernel(impl);   // weights: the PyTorch tensor (naive) or the packed one
  if (int e = run_conv(k, dtype, taps, dilation, sl, cin, (const float*)weights, tflip, weights, bias, dl, stats_partial, D(dims), S(s)))
    return e;
  if (k == ConvKernel::Naive && stats_partial) {   // (the naive conv leaves the statistics to a pass of their own)
    SEUNET_CHECK(ndst == 1, "conv3d_fwd: statistics need a single destination");
    return launch_channel_stats(dtype, dst[0], dst_c[0], stats_partial, D(dims), S(s));
  }
  return 0;
}
int seunet_conv3d_stream_supported(int dtype, int dilation, int src_c, int dst_c) { return conv_stream_supported(dtype, 27, dilation, src_c, dst_c) ? 1 : 0; }
size_t seunet_conv3d_stream_wpack_bytes(int src_c) { return conv_stream_wpack_bytes(src_c); }
int seunet_conv3d_stream_slots(int dilation, seunet_dims dims) { return conv_stream_slots(D(dims), dilation); }
int seunet_conv3d_stream_pack(int dtype, const float* w, int cin_w, int cout_w, int transpose_flip, int src_c, int dst_c, void* wpack,
                              seunet_stream_t s) {
  return pack_one(ConvKernel::Stream, dtype, w, 27, cin_w, cout_w, transpose_flip, src_c, dst_c, wpack, s);
}
int seunet_conv3d_stream(int dtype, int dilation, const void* src, int src_c, const void* wpack, const float* bias, void* dst, int dst_c,
                         int dst_accumulate, double* stats_partial, seunet_dims dims, seunet_stream_t s) {
  const SrcList sl{{src}, {src_c}, 1};
  const DstList dl{{dst}, {dst_c}, {dst_accumulate}, 1};
  return run_conv(ConvKernel::Stream, dtype, 27, dilation, sl, src_c, nullptr, 0, wpack, bias, dl, stats_partial, D(dims), S(s));
}
int seunet_conv3d_march_supported(int dtype, int dilation, int nsrc, const int* src_c, int ndst, const int* dst_c) {
  if (nsrc < 1 || nsrc > 3 || ndst < 1 || ndst > 3 || !src_c || !dst_c) return 0;   // (a query sets no error)
  SrcList sl; DstList dl;
  make_src(nsrc, nullptr, src_c, sl, true);
  make_dst(ndst, nullptr, dst_c, nullptr, dl);
  return conv_supported(ConvKernel::March, dtype, 27, dilation, sl, dl) ? 1 : 0;
}
size_t seunet_conv3d_march_wpack_bytes(int cin, int cout) { return conv_march_wpack_bytes(cin, cout); }
int seunet_conv3d_march_slots(int dilation, int cin, int cout, seunet_dims dims) { return conv_march_slots(D(dims), dilation, cin, cout); }
int seunet_conv3d_march_pack(int dtype, const float* w, int cin_w, int cout_w, int transpose_flip, int cin, int cout, void* wpack,
                             seunet_stream_t s) {
  return pack_one(ConvKernel::March, dtype, w, 27, cin_w, cout_w, transpose_flip, cin, cout, wpack, s);
}
int seunet_conv3d_march(int dtype, int dilation, int nsrc, const void* const* src, const int* src_c, const void* wpack, const float* bias,
                        int ndst, void* const* dst, const int* dst_c, const int* dst_accumulate, double* stats_partial, seunet_dims dims,
                        seunet_stream_t s) {
  SrcList sl; DstList dl;
  if (int e = make_src(nsrc, src, src_c, sl)) return e;
  SEUNET_CHECK(dst != nullptr, "conv3d_march: null destination list");
  if (int e = make_dst(ndst, dst, dst_c, dst_accumulate, dl)) return e;
  return run_conv(ConvKernel::March, dtype, 27, dilation, sl, sl.total(), nullptr, 0, wpack, bias, dl, stats_partial, D(dims), S(s));
}
int seunet_conv3d_wgrad_stream_supported(int dtype, int dilation, int x_c, int dy_c) { return wgrad_stream_supported(dtype, 27, dilation, x_c, dy_c) ? 1 : 0; }
size_t seunet_conv3d_wgrad_stream_workspace_bytes(int x_c, int dy_c, int dilation, seunet_dims dims) {
  return wgrad_stream_workspace_bytes(x_c, dy_c, dilation, D(dims));
}
int seunet_conv3d_wgrad_stream(int dtype, int dilation, const void* x, int x_c, int cin, const void* dy, int dy_c, int cout, float* dw,
                               void* workspace, size_t workspace_bytes, seunet_dims dims, seunet_stream_t s) {
  return launch_wgrad_stream(dtype, dilation, x, x_c, cin, dy, dy_c, cout, dw, workspace, workspace_bytes, D(dims), S(s));
}
size_t seunet_conv3d_wgrad_workspace_bytes(int taps, int cin, int cout) { return wgrad_workspace_bytes(taps, cin, cout); }
int seunet_conv3d_wgrad(int dtype, int impl, int taps, int dilation, int nsrc, const void* const* src, const int* src_c, int cin,
                        const void* dy, int cout, float* dw, void* workspace, size_t workspace_bytes, seunet_dims dims,
                        seunet_stream_t s) {
  SrcList sl;
  if (int e = make_src(nsrc, src, src_c, sl)) return e;
  SEUNET_CHECK(dy && dw, "conv3d_wgrad: null tensor");
  if (impl == SEUNET_CONV_NAIVE) return launch_wgrad_naive(dtype, taps, dilation, sl, cin, dy, cout, dw, D(dims), S(s));
  SEUNET_CHECK(workspace, "conv3d_wgrad: null workspace");
  // SEUNET_CONV_MARCH / SEUNET_CONV_TILED force a kernel; anything else picks by size, as the network's plan does
  const ConvKernel k = impl == SEUNET_CONV_MARCH ? (taps == 1 ? ConvKernel::Wgrad1x1 : ConvKernel::March)
                       : impl == SEUNET_CONV_TILED ? ConvKernel::Tiled
                                                   : wgrad_kernel(dtype, taps, dilation, sl, cin, cout, D(dims), sl.gap());
  return run_wgrad(k, dtype, taps, dilation, sl, cin, dy, cout, dw, workspace, workspace_bytes, D(dims), S(s));
}

int seunet_epilogue_slots(seunet_dims dims) { return epi_partials(D(dims)); }
int seunet_channel_stats(int dtype, const void* t, int c, double* partial, seunet_dims dims, seunet_stream_t s) {
  SEUNET_CHECK(t && partial, "channel_stats: null tensor");
  return launch_channel_stats(dtype, t, c, partial, D(dims), S(s));
}
int seunet_stats_finalize(const double* partial, int slots, int c, int n, long long count, float eps, int mode, float* out_a,
                          float* out_b, seunet_stream_t s) {
  SEUNET_CHECK(partial && out_a && out_b && slots >= 1 && count >= 1, "stats_finalize: bad argument");
  return launch_stats_finalize(partial, slots, c, n, count, eps, mode, out_a, out_b, S(s));
}

int seunet_gate_epilogue_fwd(int dtype, const void* raw, const float* mean, const float* rstd, int c, const float* w_se,
                             const float* w_se2, const float* w_side, const float* b_side, float slope, void* e_out,
                             float* side_out, float* level_map, int level_accumulate, const float* head_w, const float* drop,
                             int drop_stride, seunet_dims dims, seunet_stream_t s) {
  SEUNET_CHECK(raw && mean && rstd && w_se && w_side && b_side && e_out, "gate_epilogue_fwd: null tensor");
  SEUNET_CHECK(!level_map || head_w, "gate_epilogue_fwd: level_map needs head_w");
  const GateBlock b{{raw, mean, rstd}, c, {w_se, w_se2, w_side, b_side, slope}};
  SseHead h{side_out, level_map, level_accumulate, head_w, drop, drop_stride};
  return launch_sse_fwd(dtype, b, e_out, h, D(dims), S(s));
}
int seunet_gate_epilogue_bwd(int dtype, const void* raw, const float* mean, const float* rstd, int c, const float* w_se,
                             const float* w_se2, const float* w_side, const float* b_side, float slope, const void* g_e,
                             const float* g_side, const float* g_level, const float* head_w, const float* drop, int drop_stride,
                             const float* m1, const float* m2, void* draw_out, double* stat_partial, float* pgrad_partial,
                             seunet_dims dims, seunet_stream_t s) {
  SEUNET_CHECK(raw && mean && rstd && w_se && w_side && b_side, "gate_epilogue_bwd: null tensor");
  SEUNET_CHECK(!g_level || head_w, "gate_epilogue_bwd: g_level needs head_w");
  const GateBlock b{{raw, mean, rstd}, c, {w_se, w_se2, w_side, b_side, slope}};
  SseBwdIn g{g_e, g_side, g_level};
  SseHead h{nullptr, nullptr, 0, head_w, drop, drop_stride};
  if (m1 == nullptr) return launch_sse_bwd_sums(dtype, b, g, h, {stat_partial, pgrad_partial}, D(dims), S(s));   // pass A
  return launch_sse_bwd_apply(dtype, b, g, h, {m1, m2, draw_out}, D(dims), S(s));
}
int seunet_pgrad_reduce(const float* pgrad_partial, int records, int c, float* dw_se, float* dw_se2, float* dw_side,
                        float* db_side, float* dhead_w, seunet_stream_t s) {
  SEUNET_CHECK(pgrad_partial && records >= 1, "pgrad_reduce: bad argument");
  return launch_pgrad_reduce(pgrad_partial, records, c, dw_se, dw_se2, dw_side, db_side, dhead_w, S(s));
}
int seunet_gate_bwd_finalize(const double* stat_partial, int slots, int c, int n, long long count, float* m1, float* m2,
                             const float* pgrad_partial, int records, float* dw_se, float* dw_se2, float* dw_side,
                             float* db_side, float* dhead_w, seunet_stream_t s) {
  SEUNET_CHECK(stat_partial && m1 && m2 && pgrad_partial && slots >= 1 && n >= 1 && count >= 1, "gate_bwd_finalize: bad argument");
  SEUNET_CHECK(c % 8 == 0 && c >= 8 && c <= 128 && (c & (c - 1)) == 0, "channel count %d must be a power of two in [8,128]", c);
  SEUNET_CHECK(records == n * slots, "gate_bwd_finalize: records=%d, pass A wrote n * slots = %d", records, n * slots);
  return launch_gate_bwd_finalize(stat_partial, slots, c, n, count, m1, m2, pgrad_partial, records, dw_se, dw_se2, dw_side,
                                  db_side, dhead_w, S(s));
}
// the C ABI of the aggregation block's backward: m1 == nullptr asks for pass A (the sums), anything else for pass B
static int cat_epilogue_bwd(int dtype, const CatBlock& b, const void* g_out, const PoolGrad& pool, const float* m1, const float* m2,
                            const float* m1b, const float* m2b, void* dx, void* dx2, double* stat_partial, double* stat_partial2,
                            double* xw_partial, seunet_dims dims, seunet_stream_t s) {
  if (m1 == nullptr) return launch_cat_bwd_sums(dtype, b, g_out, pool, {stat_partial, stat_partial2, xw_partial}, D(dims), S(s));
  return launch_cat_bwd_apply(dtype, b, g_out, pool, {m1, m2, m1b, m2b, dx, dx2, nullptr, 0}, D(dims), S(s));
}
int seunet_cat_epilogue_fwd(int dtype, const void* raw, const float* mean, const float* rstd, const void* raw2,
                            const float* mean2, const float* rstd2, int c, float slope, void* out, seunet_dims dims,
                            seunet_stream_t s) {
  SEUNET_CHECK(raw && mean && rstd && out && (!raw2 || (mean2 && rstd2)), "cat_epilogue_fwd: null tensor");
  const CatBlock b{{raw, mean, rstd}, {raw2 ? Branch2::Stored : Branch2::None, raw2, mean2, rstd2, nullptr, 0}, c, slope};
  return launch_cat_fwd(dtype, b, out, PoolOut{}, D(dims), S(s));
}
int seunet_cat_epilogue_bwd(int dtype, const void* g_out, const void* raw, const float* mean, const float* rstd,
                            const void* raw2, const float* mean2, const float* rstd2, int c, float slope, const float* m1,
                            const float* m2, const float* m1b, const float* m2b, void* dx, void* dx2, double* stat_partial,
                            double* stat_partial2, seunet_dims dims, seunet_stream_t s) {
  SEUNET_CHECK(g_out && raw && mean && rstd, "cat_epilogue_bwd: null tensor");
  SEUNET_CHECK(!raw2 || (mean2 && rstd2), "cat_epilogue_bwd: second branch incomplete");
  const CatBlock b{{raw, mean, rstd}, {raw2 ? Branch2::Stored : Branch2::None, raw2, mean2, rstd2, nullptr, 0}, c, slope};
  return cat_epilogue_bwd(dtype, b, g_out, PoolGrad{}, m1, m2, m1b, m2b, dx, dx2, stat_partial, stat_partial2, nullptr, dims, s);
}

int seunet_maxpool_fwd(int dtype, const void* in, int c, void* out, seunet_dims d, seunet_stream_t s) {
  SEUNET_CHECK(in && out, "maxpool_fwd: null tensor");
  return launch_maxpool_fwd(dtype, in, c, out, D(d), S(s));
}
int seunet_maxpool_bwd(int dtype, const void* in, const void* g_out, int c, void* g_in, int accumulate, seunet_dims d,
                       seunet_stream_t s) {
  SEUNET_CHECK(in && g_out && g_in, "maxpool_bwd: null tensor");
  return launch_maxpool_bwd(dtype, in, g_out, c, g_in, accumulate, D(d), S(s));
}
int seunet_upsample2_fwd(int dtype, const void* in, int c, void* out, seunet_dims d, seunet_stream_t s) {
  SEUNET_CHECK(in && out, "upsample2_fwd: null tensor");
  return launch_upsample2_fwd(dtype, in, c, out, D(d), S(s));
}
int seunet_upsample2_bwd(int dtype, const void* g_out, int c, void* g_in, int accumulate, seunet_dims d, seunet_stream_t s) {
  SEUNET_CHECK(g_out && g_in, "upsample2_bwd: null tensor");
  return launch_upsample2_bwd(dtype, g_out, c, g_in, accumulate, D(d), S(s));
}
int seunet_side_upsample(const float* side, int c, int scale, float* out, int c_total, int c_off, seunet_dims low,
                         seunet_stream_t s) {
  SEUNET_CHECK(side && out && scale >= 1, "side_upsample: bad argument");
  return launch_side_upsample(side, c, scale, out, c_total, c_off, D(low), S(s));
}

int seunet_head_fwd(const float* const* level_maps, int nlevels, const float* bias, float* pred, seunet_dims d, seunet_stream_t s) {
  SEUNET_CHECK(level_maps && bias && pred, "head_fwd: null tensor");
  return launch_head_fwd(level_maps, nlevels, bias, pred, D(d), S(s));
}
size_t seunet_head_bwd_tmp_floats(seunet_dims d) { return head_bwd_tmp_floats(D(d)); }
int seunet_head_bwd(const float* g_pred, float* const* g_levels, int nlevels, float* tmp, float* g_bias, seunet_dims d,
                    seunet_stream_t s) {
  SEUNET_CHECK(g_pred && g_levels && tmp, "head_bwd: null tensor");
  return launch_head_bwd(g_pred, g_levels, nlevels, tmp, g_bias, D(d), S(s));
}

int seunet_loss_partial_floats(void) { return loss_partials() * SEUNET_LOSS_NSUMS; }
int seunet_loss_sums(const float* pred, int apply_sigmoid, const float* target, const float* weight, const float* skel,
                     long long n, float* partial, double* sums, int terms, seunet_stream_t s) {
  SEUNET_CHECK(pred && target && partial && sums && n >= 1, "loss_sums: bad argument");
  SEUNET_CHECK(terms >= 0 && terms <= 7, "loss_sums: terms=%d is not a mask of SEUNET_LOSS_DICE | _GUL | _ATR", terms);
  return launch_loss_sums(pred, apply_sigmoid, target, weight, skel, n, partial, sums, S(s), terms);
}
int seunet_loss_value(const double* sums0, double c_dice0, double c_gul0, double c_atr0, const double* sums1, double c_dice1,
                      double c_gul1, double c_atr1, float* value, seunet_stream_t s) {
  SEUNET_CHECK(sums0 && value, "loss_value: null argument");
  return launch_loss_value(sums0, c_dice0, c_gul0, c_atr0, sums1, c_dice1, c_gul1, c_atr1, value, S(s));
}
int seunet_loss_grad(const float* pred, int apply_sigmoid, const float* target, const float* weight, const float* skel,
                     long long n, const double* sums, float c_dice, float c_gul, float c_atr, float g_scale,
                     const float* g_scale_dev, float* g_pred, seunet_stream_t s) {
  SEUNET_CHECK(pred && target && sums && g_pred && n >= 1, "loss_grad: bad argument");
  return launch_loss_grad(pred, apply_sigmoid, target, weight, skel, n, sums, c_dice, c_gul, c_atr, g_scale, g_scale_dev, g_pred, S(s));
}

int seunet_loss_sample_partial_floats(int batch) {
  if (batch < 1 || batch > 65535) { fail("loss_sample_partial_floats: batch %d (1..65535)", batch); return 0; }
  return loss_sample_partials(batch) * SEUNET_LOSS_NSUMS;
}
int seunet_loss_sums_per_sample(const float* pred, int apply_sigmoid, const float* target, const float* weight, const float* skel,
                                int batch, long long n_per_sample, float* partial, double* sums, int terms, seunet_stream_t s) {
  SEUNET_CHECK(pred && target && partial && sums && n_per_sample >= 1, "loss_sums_per_sample: bad argument");
  SEUNET_CHECK(batch >= 1 && batch <= 65535, "loss_sums_per_sample: batch %d (1..65535)", batch);
  SEUNET_CHECK(terms >= 0 && terms <= 7, "loss_sums_per_sample: terms=%d is not a mask of SEUNET_LOSS_DICE | _GUL | _ATR", terms);
  return launch_loss_sums_per_sample(pred, apply_sigmoid, target, weight, skel, batch, n_per_sample, partial, sums, terms, S(s));
}
int seunet_loss_sample_values(const double* sums, int batch, double c_dice, double c_gul, double c_atr, float* values, seunet_stream_t s) {
  SEUNET_CHECK(sums && values && batch >= 1, "loss_sample_values: bad argument");
  return launch_loss_sample_values(sums, batch, c_dice, c_gul, c_atr, values, S(s));
}

size_t seunet_cldice_workspace_bytes(long long volumes, int n0, int n1, int n2, int iters, int save) {
  if (volumes < 1 || n0 < 1 || n1 < 1 || n2 < 1) { fail("cldice_workspace_bytes: empty shape (%lld volumes of (%d, %d, %d))", volumes, n0, n1, n2); return 0; }
  if (iters < 0 || iters > kCldiceMaxIters) { fail("cldice_workspace_bytes: iters=%d (0..%d)", iters, kCldiceMaxIters); return 0; }
  if ((long long)n0 * n1 * n2 >= (1ll << 31) / volumes) { fail("cldice_workspace_bytes: fewer than 2^31 voxels in all supported"); return 0; }
  return cldice_workspace_bytes(volumes, n0, n1, n2, iters, save != 0);
}
int seunet_cldice_partial_doubles(void) { return cldice_partial_doubles(); }
int seunet_soft_skeleton(const float* x, long long volumes, int n0, int n1, int n2, int iters, float* out, int save, void* workspace,
                         size_t workspace_bytes, seunet_stream_t s) {
  return launch_soft_skeleton(x, volumes, n0, n1, n2, iters, out, save != 0, workspace, workspace_bytes, S(s));
}
int seunet_cldice_sums(const float* skel_pred, const float* target, const float* skel_target, const float* pred, long long n,
                       double* partial, double* sums, seunet_stream_t s) {
  return launch_cldice_sums(skel_pred, target, skel_target, pred, n, partial, sums, S(s));
}
int seunet_cldice_value(const double* sums, double smooth, float* value, double* scalars, seunet_stream_t s) {
  return launch_cldice_value(sums, smooth, value, scalars, S(s));
}
int seunet_cldice_backward(const float* target, const float* skel_target, const double* sums, double smooth, const float* g_dev,
                           long long volumes, int n0, int n1, int n2, int iters, float* grad, void* workspace, size_t workspace_bytes,
                           seunet_stream_t s) {
  return launch_cldice_backward(target, skel_target, sums, smooth, g_dev, volumes, n0, n1, n2, iters, grad, workspace, workspace_bytes, S(s));
}
int seunet_cldice_counts(const unsigned char* skel_pred, const unsigned char* label, const unsigned char* skel_label,
                         const unsigned char* pred, long long n, unsigned long long* counts, seunet_stream_t s) {
  return launch_cldice_counts(skel_pred, label, skel_label, pred, n, counts, S(s));
}

int seunet_pool_select(const float* new_keys, int batch, float* keys, long long* seq, long long* state, int capacity, int* slots_out,
                       seunet_stream_t s) {
  return launch_pool_select(new_keys, batch, keys, seq, state, capacity, slots_out, S(s));
}
int seunet_pool_scatter(const int* slots_dev, int batch, int capacity, long long voxels, const float* data, const float* label,
                        const float* weight, const float* skel, float* pool_data, unsigned char* pool_label, float* pool_weight,
                        unsigned char* pool_skel, seunet_stream_t s) {
  return launch_pool_scatter(slots_dev, batch, capacity, voxels, data, label, weight, skel, pool_data, pool_label, pool_weight, pool_skel,
                             S(s));
}
int seunet_pool_gather(const int* slots_host, int n, int capacity, long long voxels, const float* pool_data,
                       const unsigned char* pool_label, const float* pool_weight, const unsigned char* pool_skel, float* data_out,
                       float* label_out, float* weight_out, float* skel_out, seunet_stream_t s) {
  return launch_pool_gather(slots_host, n, capacity, voxels, pool_data, pool_label, pool_weight, pool_skel, data_out, label_out,
                            weight_out, skel_out, S(s));
}

int seunet_xbranch_moment_slots(seunet_dims dims) { return xbranch_moment_slots(D(dims)); }
int seunet_xbranch_moments(int dtype, const void* x_in, double* partial, seunet_dims dims, seunet_stream_t s) {
  SEUNET_CHECK(x_in && partial, "xbranch_moments: null argument");
  return launch_xbranch_moments(dtype, x_in, partial, D(dims), S(s));
}
int seunet_xbranch_stats(const double* partial, int slots, const float* w2, int c, int in_channel, int n, long long count,
                         float eps, float* mean2, float* rstd2, double* moments_out, seunet_stream_t s) {
  SEUNET_CHECK(partial && w2 && mean2 && rstd2 && slots >= 1 && c >= 1 && n >= 1 && count >= 1, "xbranch_stats: bad argument");
  return launch_xbranch_stats(partial, slots, w2, c, in_channel, n, count, eps, mean2, rstd2, moments_out, S(s));
}
int seunet_cat_epilogue_fwd_x(int dtype, const void* raw, const float* mean, const float* rstd, const void* x_in,
                              const float* w2, int in_channel, const float* mean2, const float* rstd2, int c, float slope,
                              void* out, seunet_dims dims, seunet_stream_t s) {
  SEUNET_CHECK(raw && mean && rstd && x_in && w2 && mean2 && rstd2 && out, "cat_epilogue_fwd_x: null argument");
  const CatBlock b{{raw, mean, rstd}, {Branch2::Recomputed, x_in, mean2, rstd2, w2, in_channel}, c, slope};
  return launch_cat_fwd(dtype, b, out, PoolOut{}, D(dims), S(s));
}
int seunet_cat_epilogue_bwd_x(int dtype, const void* g_out, const void* raw, const float* mean, const float* rstd,
                              const void* x_in, const float* w2, int in_channel, const float* mean2, const float* rstd2,
                              int c, float slope, const float* m1, const float* m2, const float* m1b, const float* m2b,
                              void* dx, double* stat_partial, double* stat_partial2, double* xw_partial, seunet_dims dims,
                              seunet_stream_t s) {
  SEUNET_CHECK(g_out && raw && mean && rstd && x_in && w2 && mean2 && rstd2, "cat_epilogue_bwd_x: null argument");
  const CatBlock b{{raw, mean, rstd}, {Branch2::Recomputed, x_in, mean2, rstd2, w2, in_channel}, c, slope};
  return cat_epilogue_bwd(dtype, b, g_out, PoolGrad{}, m1, m2, m1b, m2b, dx, nullptr, stat_partial, stat_partial2, xw_partial, dims, s);
}
int seunet_cat_epilogue_fwd_x_pool(int dtype, const void* raw, const float* mean, const float* rstd, const void* x_in,
                                   const float* w2, int in_channel, const float* mean2, const float* rstd2, int c, float slope,
                                   void* out, void* pooled, unsigned int* argmax, seunet_dims dims, seunet_stream_t s) {
  SEUNET_CHECK(raw && mean && rstd && x_in && w2 && mean2 && rstd2 && out && pooled, "cat_epilogue_fwd_x_pool: null argument");
  const CatBlock b{{raw, mean, rstd}, {Branch2::Recomputed, x_in, mean2, rstd2, w2, in_channel}, c, slope};
  return launch_cat_fwd(dtype, b, out, PoolOut{pooled, argmax}, D(dims), S(s));
}
int seunet_cat_epilogue_bwd_x_pool(int dtype, const void* g_out, const void* raw, const float* mean, const float* rstd,
                                   const void* x_in, const float* w2, int in_channel, const float* mean2, const float* rstd2,
                                   int c, float slope, const float* m1, const float* m2, const float* m1b, const float* m2b,
                                   void* dx, double* stat_partial, double* stat_partial2, double* xw_partial,
                                   const unsigned int* pool_argmax, const void* pool_g, seunet_dims dims, seunet_stream_t s) {
  SEUNET_CHECK(g_out && raw && mean && rstd && x_in && w2 && mean2 && rstd2, "cat_epilogue_bwd_x_pool: null argument");
  SEUNET_CHECK((pool_argmax == nullptr) == (pool_g == nullptr), "cat_epilogue_bwd_x_pool: pool_argmax and pool_g go together");
  const CatBlock b{{raw, mean, rstd}, {Branch2::Recomputed, x_in, mean2, rstd2, w2, in_channel}, c, slope};
  return cat_epilogue_bwd(dtype, b, g_out, PoolGrad{pool_argmax, pool_g}, m1, m2, m1b, m2b, dx, nullptr, stat_partial, stat_partial2,
                          xw_partial, dims, s);
}
int seunet_cat_xgrad_finalize(const double* xw_partial, const double* stat_partial2, int slots, const double* moments, const float* w2,
                              int c, int in_channel, int n, float eps, float* dw, seunet_stream_t s) {
  SEUNET_CHECK(xw_partial && stat_partial2 && moments && w2 && dw && slots >= 1 && c >= 8 && n >= 1, "cat_xgrad_finalize: bad argument");
  return launch_cat_xgrad_finalize(xw_partial, stat_partial2, slots, moments, w2, c, in_channel, n, eps, dw, S(s));
}

size_t seunet_cc_workspace_bytes(int h, int w, int z) {
  if (h < 1 || w < 1 || z < 1) { fail("cc_workspace_bytes: bad dimensions"); return 0; }
  return cc_workspace_bytes(h, w, z);
}
int seunet_largest_component(const unsigned char* volume, int h, int w, int z, int rule, unsigned char* out, int* status_dev,
                             void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  return launch_largest_component(volume, h, w, z, rule, out, status_dev, workspace, workspace_bytes, S(s));
}
size_t seunet_metric_out_bytes(int nbins) { return nbins < 1 ? 0 : metric_out_bytes(nbins); }
int seunet_metric_sums(const unsigned char* pred, const unsigned char* label, const unsigned char* skeleton, const int* parsing,
                       long long n, int nbins, void* out, size_t out_bytes, seunet_stream_t s) {
  return launch_metric_sums(pred, label, skeleton, parsing, n, nbins, out, out_bytes, S(s));
}

size_t seunet_edt_workspace_bytes(int n0, int n1, int n2) {
  if (n0 < 1 || n1 < 1 || n2 < 1) { fail("edt_workspace_bytes: bad dimensions"); return 0; }
  return edt_workspace_bytes(n0, n1, n2);
}
int seunet_edt(const unsigned char* volume, int n0, int n1, int n2, int* sqdist, double* dist, int* indices, int* status_dev,
               void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  return launch_edt(volume, n0, n1, n2, sqdist, dist, indices, status_dev, workspace, workspace_bytes, S(s));
}
size_t seunet_edt_sampling_workspace_bytes(int n0, int n1, int n2) {
  if (n0 < 1 || n1 < 1 || n2 < 1) { fail("edt_sampling_workspace_bytes: bad dimensions"); return 0; }
  return edt_sampling_workspace_bytes(n0, n1, n2);
}
int seunet_edt_sampling(const unsigned char* volume, int n0, int n1, int n2, double s0, double s1, double s2, double* dist, int* indices,
                        int* lin, int* status_dev, void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  return launch_edt_sampling(volume, n0, n1, n2, s0, s1, s2, EdtSamplingOut{dist, indices, lin}, status_dev, workspace, workspace_bytes,
                             S(s));
}
int seunet_mask_bits(const unsigned char* mask, long long n, unsigned long long* bits, seunet_stream_t s) {
  return launch_mask_bits(mask, n, bits, S(s));
}
int seunet_hard_mining_masks(const unsigned char* label, const unsigned char* skeleton, const unsigned char* pred, int n0, int n1,
                             int n2, unsigned long long* skeleton_bits, unsigned long long* small_bits, seunet_stream_t s) {
  return launch_hm_candidates(label, skeleton, pred, n0, n1, n2, skeleton_bits, small_bits, S(s));
}
size_t seunet_lib_weight_workspace_bytes(int n0, int n1, int n2) {
  if (n0 < 1 || n1 < 1 || n2 < 1) { fail("lib_weight_workspace_bytes: bad dimensions"); return 0; }
  return lib_weight_workspace_bytes(n0, n1, n2);
}
int seunet_lib_weight(const unsigned char* label, int n0, int n1, int n2, const float* table, void* out, void* workspace,
                      size_t workspace_bytes, seunet_stream_t s) {
  return launch_lib_weight(label, n0, n1, n2, table, out, workspace, workspace_bytes, S(s));
}
size_t seunet_break_weight_workspace_bytes(int n0, int n1, int n2) {
  if (n0 < 1 || n1 < 1 || n2 < 1) { fail("break_weight_workspace_bytes: bad dimensions"); return 0; }
  return break_weight_workspace_bytes(n0, n1, n2);
}
int seunet_break_weight(const unsigned char* label, const unsigned char* pred, const unsigned char* skeleton, int n0, int n1, int n2,
                        void* w_br, unsigned char* br_skel, int* status_dev, void* workspace, size_t workspace_bytes,
                        seunet_stream_t s) {
  return launch_break_weight(label, pred, skeleton, n0, n1, n2, w_br, br_skel, status_dev, workspace, workspace_bytes, S(s));
}

size_t seunet_skeleton_workspace_bytes(int n0, int n1, int n2) {
  const size_t bytes = skeleton_workspace_bytes(n0, n1, n2);
  if (bytes == 0) fail("skeleton_workspace_bytes: bad dimensions (%d, %d, %d): extents >= 1, at most 2^31-1 voxels", n0, n1, n2);
  return bytes;
}
int seunet_skeletonize(const unsigned char* volume, int n0, int n1, int n2, unsigned char* out, int* passes_dev, void* workspace,
                       size_t workspace_bytes, seunet_stream_t s) {
  return launch_skeletonize(volume, n0, n1, n2, out, passes_dev, workspace, workspace_bytes, S(s));
}

size_t seunet_skeleton_branches_workspace_bytes(int n0, int n1, int n2) {
  if (n0 < 1 || n1 < 1 || n2 < 1 || (long long)n0 * n1 * n2 >= (1ll << 31)) { fail("skeleton_branches_workspace_bytes: bad dimensions"); return 0; }
  return skeleton_branches_workspace_bytes(n0, n1, n2);
}
int seunet_skeleton_branches(const unsigned char* skeleton, int n0, int n1, int n2, int min_voxels, int* cd, unsigned char* skeleton_parse,
                             int* num_dev, void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  return launch_skeleton_branches(skeleton, n0, n1, n2, min_voxels, cd, skeleton_parse, num_dev, workspace, workspace_bytes, S(s));
}
size_t seunet_parse_assign_workspace_bytes(int n0, int n1, int n2) {
  if (n0 < 1 || n1 < 1 || n2 < 1) { fail("parse_assign_workspace_bytes: bad dimensions"); return 0; }
  return parse_assign_workspace_bytes(n0, n1, n2);
}
int seunet_parse_assign(const unsigned char* skeleton_parse, const int* cd, const unsigned char* label, int n0, int n1, int n2,
                        int* parsing, int* status_dev, void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  return launch_parse_assign(skeleton_parse, cd, label, n0, n1, n2, parsing, status_dev, workspace, workspace_bytes, S(s));
}
int seunet_label_stats_max_num(void) { return label_stats_max_num(); }
int seunet_label_stats(const int* parsing, int n0, int n1, int n2, int num, unsigned int* counts, unsigned long long* adjacency_bits,
                       int* status_dev, seunet_stream_t s) {
  return launch_label_stats(parsing, n0, n1, n2, num, counts, adjacency_bits, status_dev, S(s));
}
int seunet_relabel(const int* parsing, long long n, const int* lut, int nlut, int* out, seunet_stream_t s) {
  return launch_relabel(parsing, n, lut, nlut, out, S(s));
}

size_t seunet_binary_morph_workspace_bytes(int n0, int n1, int n2) {
  if (n0 < 1 || n1 < 1 || n2 < 1) { fail("binary_morph_workspace_bytes: bad dimensions"); return 0; }
  return binary_morph_workspace_bytes(n0, n1, n2);
}
int seunet_binary_morph(const unsigned char* volume, int n0, int n1, int n2, int op, unsigned char* out, void* workspace,
                        size_t workspace_bytes, seunet_stream_t s) {
  return launch_binary_morph(volume, n0, n1, n2, op, out, workspace, workspace_bytes, S(s));
}
int seunet_fill_holes(const unsigned char* volume, int n0, int n1, int n2, unsigned char* out, void* workspace, size_t workspace_bytes,
                      seunet_stream_t s) {
  return launch_fill_holes(volume, n0, n1, n2, out, workspace, workspace_bytes, S(s));
}
int seunet_slice_moments(const unsigned char* mask, int n0, int n1, int n2, int k, unsigned long long* out_dev, seunet_stream_t s) {
  return launch_slice_moments(mask, n0, n1, n2, k, out_dev, S(s));
}
int seunet_scatter_labels(const long long* lin_index_dev, const int* value_dev, long long m, long long n, int* cd,
                          unsigned char* skeleton_parse, int* status_dev, seunet_stream_t s) {
  return launch_scatter_labels(lin_index_dev, value_dev, m, n, cd, skeleton_parse, status_dev, S(s));
}

size_t seunet_mesh_workspace_bytes(int n0, int n1, int n2) {
  if (volume_check("mesh_workspace_bytes", n0, n1, n2, 0)) return 0;
  return mesh_workspace_bytes(n0, n1, n2);
}
int seunet_mesh_count(const unsigned char* volume, int n0, int n1, int n2, long long* nverts, long long* nfaces, void* workspace,
                      size_t workspace_bytes, seunet_stream_t s) {
  return launch_mesh_count(volume, n0, n1, n2, nverts, nfaces, workspace, workspace_bytes, S(s));
}
int seunet_mesh_emit(int n0, int n1, int n2, double level, long long nverts, long long nfaces, float* verts, int* faces,
                     const void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  return launch_mesh_emit(n0, n1, n2, level, nverts, nfaces, verts, faces, workspace, workspace_bytes, S(s));
}
size_t seunet_mesh_label_workspace_bytes(int n0, int n1, int n2) {
  if (volume_check("mesh_label_workspace_bytes", n0, n1, n2, 0)) return 0;
  return mesh_label_workspace_bytes(n0, n1, n2);
}
size_t seunet_mesh_label_sort_bytes(long long nverts, long long nfaces) {
  if (nverts < 0 || nfaces < 0 || nverts > 0x7fffffffll || 3 * nfaces > 0x7fffffffll) {
    fail("mesh_label_sort_bytes: bad sizes (%lld vertices, %lld faces)", nverts, nfaces);
    return 0;
  }
  return mesh_label_sort_bytes(nverts, nfaces);
}
int seunet_mesh_label_count(const int* labels, int n0, int n1, int n2, int num, long long* nverts, long long* nfaces, int* num_used,
                            int* status, long long* vert_ptr_dev, long long* face_ptr_dev, int ptr_capacity, void* workspace,
                            size_t workspace_bytes, seunet_stream_t s) {
  return launch_mesh_label_count(labels, n0, n1, n2, num, nverts, nfaces, num_used, status, vert_ptr_dev, face_ptr_dev, ptr_capacity,
                                 workspace, workspace_bytes, S(s));
}
int seunet_mesh_label_emit(const int* labels, int n0, int n1, int n2, int num, double level, long long nverts, long long nfaces,
                           float* verts, int* faces, const void* workspace, size_t workspace_bytes, void* sort_workspace,
                           size_t sort_bytes, seunet_stream_t s) {
  return launch_mesh_label_emit(labels, n0, n1, n2, num, level, nverts, nfaces, verts, faces, workspace, workspace_bytes,
                                sort_workspace, sort_bytes, S(s));
}
int seunet_branch_stats(const int* parsing, const unsigned char* skeleton, const int* sqdist, int n0, int n1, int n2, int num,
                        long long* voxels, long long* coord_sum, int* box_min, int* box_max, long long* skeleton_voxels, long long* links,
                        long long* cross_links, long long* r2_sum, int* r2_min, int* r2_max, int* status_dev, seunet_stream_t s) {
  return launch_branch_stats(parsing, skeleton, sqdist, n0, n1, n2, num,
                             BranchStatsOut{voxels, coord_sum, box_min, box_max, skeleton_voxels, links, cross_links, r2_sum, r2_min,
                                            r2_max, status_dev},
                             S(s));
}
int seunet_branch_wall_stats(const int* parsing, const unsigned char* skeleton, const int* indices, int n0, int n1, int n2, int num,
                             double s0, double s1, double s2, long long* wall_count, long long* offset_sq_sum, double* wall_sq_min,
                             double* wall_sq_max, int* status_dev, seunet_stream_t s) {
  return launch_branch_wall_stats(parsing, skeleton, indices, n0, n1, n2, num, s0, s1, s2,
                                  BranchWallOut{wall_count, offset_sq_sum, wall_sq_min, wall_sq_max, status_dev}, S(s));
}
size_t seunet_cross_section_workspace_bytes(int n0, int n1, int n2) {
  if (volume_check("cross_section_workspace_bytes", n0, n1, n2, 0)) return 0;
  return cross_section_workspace_bytes(n0, n1, n2);
}
int seunet_cross_section_sweep_points(void) { return cross_section_sweep_points(); }
int seunet_cross_section_count(const int* parsing, const unsigned char* skeleton, int n0, int n1, int n2, int num, long long* m, int* status,
                               void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  return launch_cross_section_count(parsing, skeleton, n0, n1, n2, num, m, status, workspace, workspace_bytes, S(s));
}
int seunet_cross_section_emit(const int* parsing, const unsigned char* skeleton, int n0, int n1, int n2, double s0, double s1, double s2,
                              double step, int window, int same_label, long long m, int* lin, double* tangent, int* table,
                              const void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  return launch_cross_section_emit(parsing, skeleton, n0, n1, n2, s0, s1, s2, step, window, same_label, m, lin, tangent, table, workspace,
                                   workspace_bytes, S(s));
}
int seunet_airway_wall_rays(void) { return airway_wall_rays(); }
int seunet_airway_wall_samples(void) { return airway_wall_samples(); }
int seunet_airway_wall_sweep_points(void) { return airway_wall_sweep_points(); }
int seunet_airway_wall_directions(double* out) {
  SEUNET_CHECK(out, "airway_wall_directions: null argument");
  airway_wall_directions(out);
  return 0;
}
int seunet_airway_walls(const void* ct, int ct_dtype, const int* parsing, int n0, int n1, int n2, double s0, double s1, double s2,
                        double step, double ray_step, int n_search, float min_contrast, int same_label, long long m, const int* table,
                        const double* tangent, unsigned long long* mask, double* sums, unsigned char* codes, double* edges,
                        seunet_stream_t s) {
  return launch_airway_walls(ct, ct_dtype, parsing, n0, n1, n2, s0, s1, s2, step, ray_step, n_search, min_contrast, same_label, m, table,
                             tangent, mask, sums, codes, edges, S(s));
}
size_t seunet_surface_workspace_bytes(int n0, int n1, int n2) {
  if (volume_check("surface_workspace_bytes", n0, n1, n2, kEdtMaxExtent)) return 0;
  return surface_workspace_bytes(n0, n1, n2);
}
int seunet_surface_count(const unsigned char* a, const unsigned char* b, int n0, int n1, int n2, long long* n_a, long long* n_b, int* box,
                         void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  return launch_surface_count(a, b, n0, n1, n2, n_a, n_b, box, workspace, workspace_bytes, S(s));
}
size_t seunet_surface_emit_workspace_bytes(int b0, int b1, int b2) {
  if (volume_check("surface_emit_workspace_bytes", b0, b1, b2, kEdtMaxExtent)) return 0;
  return surface_emit_workspace_bytes(b0, b1, b2);
}
int seunet_surface_emit(int n0, int n1, int n2, const int* box, double s0, double s1, double s2, long long n_a, long long n_b,
                        double* dist, int* voxel, const void* count_workspace, size_t count_workspace_bytes, void* emit_workspace,
                        size_t emit_workspace_bytes, seunet_stream_t s) {
  return launch_surface_emit(n0, n1, n2, box, s0, s1, s2, n_a, n_b, dist, voxel, count_workspace, count_workspace_bytes, emit_workspace,
                             emit_workspace_bytes, S(s));
}
size_t seunet_surface_summary_bytes(int ntol) {
  if (ntol < 0 || ntol > kSurfaceMaxTol) { fail("surface_summary_bytes: %d tolerances: 0 .. %d are supported", ntol, kSurfaceMaxTol); return 0; }
  return surface_summary_bytes(ntol);
}
int seunet_surface_summary(const double* dist, long long n_a, long long n_b, const double* tol, int ntol, void* out_dev,
                           seunet_stream_t s) {
  return launch_surface_summary(dist, n_a, n_b, tol, ntol, out_dev, S(s));
}
size_t seunet_select_ranks_workspace_bytes(int nranks) {
  if (nranks < 1 || nranks > kSelectMaxRanks) { fail("select_ranks_workspace_bytes: %d requests: 1 .. %d are supported", nranks, kSelectMaxRanks); return 0; }
  return select_ranks_workspace_bytes(nranks);
}
int seunet_select_ranks(const double* values, long long n, const long long* seg_begin, const long long* seg_end, const long long* rank,
                        int nranks, double* out_dev, void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  return launch_select_ranks(values, n, seg_begin, seg_end, rank, nranks, out_dev, workspace, workspace_bytes, S(s));
}
size_t seunet_label_workspace_bytes(int n0, int n1, int n2) {
  if (volume_check("label_workspace_bytes", n0, n1, n2, 0)) return 0;
  return label_workspace_bytes(n0, n1, n2);
}
int seunet_label(const unsigned char* mask, int n0, int n1, int n2, int connectivity, int* labels, int* num_dev, void* workspace,
                 size_t workspace_bytes, seunet_stream_t s) {
  return launch_label(mask, n0, n1, n2, connectivity, labels, num_dev, workspace, workspace_bytes, S(s));
}
int seunet_component_table(const int* labels, int n0, int n1, int n2, long long num, long long* size, long long* first, int* box,
                           void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  return launch_component_table(labels, n0, n1, n2, num, size, first, box, workspace, workspace_bytes, S(s));
}
int seunet_remove_small_objects(const unsigned char* mask, int n0, int n1, int n2, long long min_size, int connectivity,
                                unsigned char* out, void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  return launch_remove_small(mask, n0, n1, n2, min_size, connectivity, out, workspace, workspace_bytes, S(s));
}
// the patch of the tile calls: at least 1 per axis; an extent past the volume's is the volume's
static int patch_check(const char* what, int n0, int n1, int n2, int p0, int p1, int p2) {
  if (volume_check(what, n0, n1, n2, 0)) return 1;
  SEUNET_CHECK(p0 >= 1 && p1 >= 1 && p2 >= 1, "%s: bad patch (%d, %d, %d)", what, p0, p1, p2);
  return 0;
}
size_t seunet_euler_workspace_bytes(int n0, int n1, int n2, int p0, int p1, int p2) {
  if (patch_check("euler_workspace_bytes", n0, n1, n2, p0, p1, p2)) return 0;
  return euler_workspace_bytes(n0, n1, n2, tile_cut(n0, n1, n2, p0, p1, p2));
}
int seunet_euler(const unsigned char* mask, int n0, int n1, int n2, int p0, int p1, int p2, int connectivity, long long* chi_dev,
                 void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  if (patch_check("euler", n0, n1, n2, p0, p1, p2)) return 1;
  return launch_euler(mask, n0, n1, n2, tile_cut(n0, n1, n2, p0, p1, p2), connectivity, chi_dev, workspace, workspace_bytes, S(s));
}
size_t seunet_betti_workspace_bytes(int n0, int n1, int n2, int p0, int p1, int p2) {
  if (patch_check("betti_workspace_bytes", n0, n1, n2, p0, p1, p2)) return 0;
  return betti_workspace_bytes(n0, n1, n2, tile_cut(n0, n1, n2, p0, p1, p2));
}
int seunet_betti(const unsigned char* mask, int n0, int n1, int n2, int p0, int p1, int p2, int connectivity, int* table_dev,
                 void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  if (patch_check("betti", n0, n1, n2, p0, p1, p2)) return 1;
  return launch_betti(mask, n0, n1, n2, tile_cut(n0, n1, n2, p0, p1, p2), connectivity, table_dev, workspace, workspace_bytes, S(s));
}
int seunet_mesh_coord_sums(const unsigned char* mask, int n0, int n1, int n2, long long* sums_dev, seunet_stream_t s) {
  return launch_mesh_coord_sums(mask, n0, n1, n2, sums_dev, S(s));
}
size_t seunet_mesh_adjacency_workspace_bytes(long long nverts, long long nfaces) {
  if (nverts < 0 || nfaces < 0 || nverts > 0x7ffffffell || 6 * nfaces > 0x7fffffffll) {
    fail("mesh_adjacency_workspace_bytes: bad sizes (%lld vertices, %lld faces)", nverts, nfaces);
    return 0;
  }
  return mesh_adjacency_workspace_bytes(nverts, nfaces);
}
int seunet_mesh_adjacency(const int* faces, long long nfaces, long long nverts, int* indptr, int* indices, long long indices_capacity,
                          unsigned char* boundary, int* status_dev, void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  return launch_mesh_adjacency(faces, nfaces, nverts, indptr, indices, indices_capacity, boundary, status_dev, workspace, workspace_bytes,
                               S(s));
}
int seunet_mesh_smooth(const float* verts, long long nverts, const int* indptr, const int* indices, const unsigned char* boundary,
                       int n_iter, float relaxation_factor, float* out, float* tmp, seunet_stream_t s) {
  return launch_mesh_smooth(verts, nverts, indptr, indices, boundary, n_iter, relaxation_factor, out, tmp, S(s));
}
int seunet_mesh_affine(const float* verts, long long nverts, const float* centre, const float* scale, float* out, seunet_stream_t s) {
  return launch_mesh_affine(verts, nverts, centre, scale, out, S(s));
}
int seunet_mesh_stl_records(const float* verts, long long nverts, const int* faces, long long nfaces, const float* centre,
                            const float* scale, unsigned char* records, int* status_dev, seunet_stream_t s) {
  return launch_mesh_stl_records(verts, nverts, faces, nfaces, centre, scale, records, status_dev, S(s));
}

int seunet_value_counts(const short* ct, long long n, int shift, unsigned int* counts, seunet_stream_t s) {
  return launch_value_counts(ct, n, shift, counts, S(s));
}
int seunet_shift_clamp(const short* ct, long long n, int shift, int clamp, int clamp_le, int clamp_to, short* out, seunet_stream_t s) {
  return launch_shift_clamp(ct, n, shift, clamp, clamp_le, clamp_to, out, S(s));
}
size_t seunet_get_l_workspace_bytes(int h, int w, int z) {
  if (h < 1 || w < 1 || z < 1) { fail("get_l_workspace_bytes: bad dimensions"); return 0; }
  return get_l_workspace_bytes(h, w, z);
}
int seunet_get_l(const short* ct, int h, int w, int z, double T, int min_area, unsigned char* out, void* workspace,
                 size_t workspace_bytes, seunet_stream_t s) {
  return launch_get_l(ct, h, w, z, T, min_area, out, workspace, workspace_bytes, S(s));
}
int seunet_mask_combine(const unsigned char* a, const unsigned char* b, long long n, int op, unsigned char* out, seunet_stream_t s) {
  return launch_mask_combine(a, b, n, op, out, S(s));
}
int seunet_mask_box(const unsigned char* mask, int h, int w, int z, int* box_dev, seunet_stream_t s) {
  return launch_mask_box(mask, h, w, z, box_dev, S(s));
}
int seunet_crop3d(const void* src, int elem_bytes, int h, int w, int z, const int* box, void* dst, seunet_stream_t s) {
  return launch_crop3d(src, elem_bytes, h, w, z, box, dst, S(s));
}

int seunet_crop_batch(const void* img, int img_dtype, const unsigned char* label, const void* weight, int weight_dtype,
                      const unsigned char* skeleton, int d, int h, int w, int cube, int ncrop, const int* starts, const int* aug,
                      double weight_exponent, int f64_math, float* data_out, float* label_out, float* weight_out, float* skel_out,
                      seunet_stream_t s) {
  return launch_crop_batch(img, img_dtype, label, weight, weight_dtype, skeleton, d, h, w, cube, ncrop, starts, aug, weight_exponent,
                           f64_math, data_out, label_out, weight_out, skel_out, S(s));
}
int seunet_hu_two_channel(const void* img, int img_dtype, long long nvox, int f64_math, float* out, seunet_stream_t s) {
  return launch_hu_two_channel(img, img_dtype, nvox, f64_math, out, S(s));
}

int seunet_window_gather(const float* volume, int c, int x, int y, int z, int cube, int nwin, const int* starts, float* out,
                         seunet_stream_t s) {
  return launch_window_gather(volume, c, x, y, z, cube, nwin, starts, out, S(s));
}
int seunet_window_accumulate(const float* logits, int apply_sigmoid, int nwin, const int* starts, int cube, double* acc, int x, int y,
                             int z, seunet_stream_t s) {
  return launch_window_accumulate(logits, apply_sigmoid, nwin, starts, cube, acc, x, y, z, S(s));
}
int seunet_window_finalize(const double* acc, int x, int y, int z, int cube, int nx, const int* xs, int ny, const int* ys, int nz,
                           const int* zs, int dup0, double* out, seunet_stream_t s) {
  return launch_window_finalize(acc, x, y, z, cube, nx, xs, ny, ys, nz, zs, dup0, out, S(s));
}

size_t seunet_dti_workspace_bytes(int h, int w, int z) {
  if (h < 1 || w < 1 || z < 1) { fail("dti_workspace_bytes: bad dimensions"); return 0; }
  return dti_workspace_bytes(h, w, z);
}
int seunet_dti(const double* pred, int h, int w, int z, double h_thresh, double l_thresh, int pred_dtype, unsigned char* out,
               void* workspace, size_t workspace_bytes, seunet_stream_t s) {
  return launch_dti(pred, h, w, z, h_thresh, l_thresh, pred_dtype, out, workspace, workspace_bytes, S(s));
}

int seunet_adamw_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                      const long long* counts, int n_tensors, double lr, double beta1, double beta2, double eps,
                      double weight_decay, int step, int maximize, seunet_stream_t s) {
  SEUNET_CHECK(n_tensors == 0 || (params && grads && exp_avg && exp_avg_sq && counts), "adamw_step: bad argument");
  return launch_adamw(params, grads, exp_avg, exp_avg_sq, counts, n_tensors, lr, beta1, beta2, eps, weight_decay, step,
                      maximize, S(s));
}
int seunet_adamw_step_gated(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                            const long long* counts, const int* steps, float* const* skipped, int n_tensors, double lr,
                            double beta1, double beta2, double eps, double weight_decay, int maximize, const int* skip_flag,
                            float* table, seunet_stream_t s) {
  SEUNET_CHECK(n_tensors == 0 || (params && grads && exp_avg && exp_avg_sq && counts && steps && skipped && table),
               "adamw_step_gated: bad argument");
  return launch_adamw_gated(params, grads, exp_avg, exp_avg_sq, counts, steps, skipped, n_tensors, lr, beta1, beta2, eps,
                            weight_decay, maximize, skip_flag, table, S(s));
}

}  // extern "C"
