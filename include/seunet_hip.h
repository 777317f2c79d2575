/* seunet_hip.h -- C ABI of libseunet_hip.so: the MI355X (gfx950) SE-UNet hot path.
 *
 * The reference (Beryl2000/SE-UNet-AirSeg) has no native / FFI layer: its boundary for this path is
 * the Python nn.Module surface of SE_UNet.py plus three loss functions in train.py.
 * This header is the C boundary a binding for that surface talks to; every entry point names the
 * reference code it replaces.  Conventions:
 *   - plain C, no torch types: raw device pointers, explicit shapes, a dtype enum, a hipStream_t;
 *   - every function returns 0 on success, non-zero on error (message: seunet_last_error(), thread
 *     local); nothing throws across the ABI; every tensor and workspace is caller-owned and the
 *     launches themselves neither allocate nor synchronise;
 *   - all device work of a call (kernels, memsets, copies) is ordered on its stream argument and on nothing else, and a call
 *     that returns host values (pass counts, status words, counts, boxes) waits for that stream only;
 *   - what the library keeps per process, all of it created lazily on first need and none of it per call:
 *       (1) per device, one 4-KB page of zeros (hipMalloc + hipMemset + a wait for the null stream, so the zeros are in
 *           memory before any stream reads them: one device synchronisation, the first time a kernel that pads through it
 *           runs on that device -- or up front by seunet_init);
 *       (2) per kernel instantiation, a bit mask of the devices on which hipFuncSetAttribute (LDS above 64 KB) has run;
 *       (3) the opt-in seunet_prof_* recorder (process-wide, off by default; the per-launch-group timer of bench.py).
 *     Apart from these everything is parameterised by (pointers, stream) and calls are re-entrant across threads and
 *     streams; a graph object (seunet_net_forward_capture) is owned by the caller like any other handle;
 *   - activations inside the library are channels-last [N][D][H][W][C], C a multiple of 8, f32, bf16 or
 *     f16 (SEUNET_F32 / SEUNET_BF16 / SEUNET_F16); parameters, logits, losses and gradients of parameters are
 *     f32 in the PyTorch layouts of the reference's state_dict.
 */
#ifndef SEUNET_HIP_H
#define SEUNET_HIP_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef SEUNET_F32
#define SEUNET_F32 0
#define SEUNET_BF16 1
#define SEUNET_F16 2   /* IEEE half activation storage (BASELINE configs[4] "fp16+MFMA"): v_mfma_*_f16, same rate and bytes as bf16 */
#endif
#define SEUNET_CONV_MFMA 0   /* implicit-GEMM matrix-core kernels (default)                  */
#define SEUNET_CONV_NAIVE 1  /* one-thread-per-output HIP kernels (device-side cross-check)  */
#define SEUNET_CONV_MARCH 2  /* seunet_conv3d_wgrad only: force the marching weight-gradient kernel (taps 27) / the whole-GEMM
                                1x1x1 kernel (taps 1); SEUNET_CONV_MFMA picks them by itself for the layers and sizes they
                                win on; error when the layer is not served */
#define SEUNET_CONV_TILED 3  /* seunet_conv3d_wgrad only: the tiled weight-gradient kernel whatever the size                */

typedef void* seunet_stream_t; /* a hipStream_t */
typedef struct seunet_dims { int n, d, h, w; } seunet_dims;

int seunet_version(void);
const char* seunet_last_error(void);
/* Optional: create the per-device state (1) above for `device` now, so that no later call synchronises the device
 * (call it before stream capture or a timed region; the training / inference entry points work without it). */
int seunet_init(int device);

/* ---- layout: reference tensors are NCDHW f32 (SE_UNet.py:181 "x: 1 2 128 128 128") ---------------- */
int seunet_pack_cl(int dtype, const float* in_ncdhw, int c, void* out_cl, int c_pad, seunet_dims dims, seunet_stream_t s);
int seunet_unpack_cl(int dtype, const void* in_cl, int c, float* out_ncdhw, seunet_dims dims, seunet_stream_t s);

/* ---- nn.Conv3d 3x3x3 (dilation 1|2, padding = dilation) and 1x1x1; SE_UNet.py:15,42,57 -------------
 * src/dst lists realise torch.cat (SE_UNet.py:186,195,204,212,216,218,222,224,228) and its backward.
 * weights: SEUNET_CONV_MFMA -> buffer produced by seunet_conv_pack_weights; SEUNET_CONV_NAIVE -> the
 * PyTorch (Cout,Cin,k,k,k) f32 tensor.  transpose_flip=1 selects the data-gradient operator.
 * stats_partial (optional): [n][seunet_conv_stats_slots][cout][2] f64 partial (sum, sum of squares) for the
 * following InstanceNorm3d (SE_UNet.py:17,43,59).  f64 because var = E[x^2]-E[x]^2 must survive |mean| >> std
 * (the CPU reference accumulates in double); the network's gradient is ill-conditioned w.r.t. such errors. */
size_t seunet_conv_wpack_bytes(int dtype, int taps, int cin, int cout);
int seunet_conv_pack_weights(int dtype, const float* w, int taps, int cin, int cout, int transpose_flip, void* wpack, seunet_stream_t s);
int seunet_conv_stats_slots(int impl, int taps, int dilation, seunet_dims dims);
int seunet_conv3d_fwd(int dtype, int impl, int taps, int dilation, int nsrc, const void* const* src, const int* src_c,
                      int cin, const void* weights, int transpose_flip, const float* bias, int ndst, void* const* dst,
                      const int* dst_c, const int* dst_accumulate, double* stats_partial, seunet_dims dims, seunet_stream_t s);
/* Streaming variant of the 3x3x3 convolution for the small-channel full-resolution layers (ec1 / ec2 / ec3 / dc6 forward and
 * data gradient; SE_UNet.py:108-110,147): one source tensor of 8 / 16 / 32 channels, one destination of <= 32 (16 when the
 * source has 32) channels, bf16, dilation 1 | 2.  A workgroup marches along z with the input planes arriving by LDS-DMA
 * (csrc/conv_stream.hip).  Weights: seunet_conv3d_stream_pack (transpose_flip = 1: data-gradient operator).  stats_partial:
 * [n][seunet_conv3d_stream_slots][dst_c][2] f64 (optional), same meaning as for seunet_conv3d_fwd. */
int seunet_conv3d_stream_supported(int dtype, int dilation, int src_c, int dst_c);
size_t seunet_conv3d_stream_wpack_bytes(int src_c);
int seunet_conv3d_stream_slots(int dilation, seunet_dims dims);
int seunet_conv3d_stream_pack(int dtype, const float* w, int cin_w, int cout_w, int transpose_flip, int src_c, int dst_c, void* wpack,
                              seunet_stream_t s);
int seunet_conv3d_stream(int dtype, int dilation, const void* src, int src_c, const void* wpack, const float* bias, void* dst, int dst_c,
                         int dst_accumulate, double* stats_partial, seunet_dims dims, seunet_stream_t s);
/* The same reference op (nn.Conv3d 3x3x3, SE_UNet.py:15,57, with the torch.cat of :222,228 fused) for the 32- and 64-input-channel
 * layers of the fine levels, forward and data gradient, on the marching kernel (csrc/conv_march.hip): bf16 | f16, one or two
 * source tensors of equal channel count (32 or 64 channels together), destinations in multiples of 16 channels (32 or more
 * together; a null destination drops its channels), dilation 1 | 2.  Weights: seunet_conv3d_march_pack (transpose_flip = 1:
 * data-gradient operator).  bias / stats_partial ([n][seunet_conv3d_march_slots][cout][2] f64) belong to the forward form,
 * dst_accumulate (+=) to the data-gradient form. */
int seunet_conv3d_march_supported(int dtype, int dilation, int nsrc, const int* src_c, int ndst, const int* dst_c);
size_t seunet_conv3d_march_wpack_bytes(int cin, int cout);
int seunet_conv3d_march_slots(int dilation, int cin, int cout, seunet_dims dims);
int seunet_conv3d_march_pack(int dtype, const float* w, int cin_w, int cout_w, int transpose_flip, int cin, int cout, void* wpack,
                             seunet_stream_t s);
int seunet_conv3d_march(int dtype, int dilation, int nsrc, const void* const* src, const int* src_c, const void* wpack, const float* bias,
                        int ndst, void* const* dst, const int* dst_c, const int* dst_accumulate, double* stats_partial, seunet_dims dims,
                        seunet_stream_t s);
/* weight gradient of the same small-channel layers on the streaming structure (csrc/wgrad_stream.hip): x (x_c = 8 | 16 | 32
 * channels, cin of them carry weights), dy (dy_c channels, cout valid); dw: (cout, cin, 3, 3, 3) f32, overwritten. */
int seunet_conv3d_wgrad_stream_supported(int dtype, int dilation, int x_c, int dy_c);
size_t seunet_conv3d_wgrad_stream_workspace_bytes(int x_c, int dy_c, int dilation, seunet_dims dims);
int seunet_conv3d_wgrad_stream(int dtype, int dilation, const void* x, int x_c, int cin, const void* dy, int dy_c, int cout, float* dw,
                               void* workspace, size_t workspace_bytes, seunet_dims dims, seunet_stream_t s);
size_t seunet_conv3d_wgrad_workspace_bytes(int taps, int cin, int cout);
int seunet_conv3d_wgrad(int dtype, int impl, int taps, int dilation, int nsrc, const void* const* src, const int* src_c,
                        int cin, const void* dy, int cout, float* dw, void* workspace, size_t workspace_bytes,
                        seunet_dims dims, seunet_stream_t s);

/* ---- InstanceNorm3d statistics (eps, biased variance; SE_UNet.py:17,43,59) -------------------------- */
int seunet_epilogue_slots(seunet_dims dims);
int seunet_channel_stats(int dtype, const void* t, int c, double* partial, seunet_dims dims, seunet_stream_t s);
/* mode 0: (mean, rstd) ; mode 1: (sum/count, sumsq/count) */
int seunet_stats_finalize(const double* partial, int slots, int c, int n, long long count, float eps, int mode,
                          float* out_a, float* out_b, seunet_stream_t s);

/* ---- gated block epilogue: IN -> LeakyReLU -> gate(s) -> e, side = conv1x1(e); SE_UNet.py:24-35,68-82 --
 * w_se2 == NULL selects the one-gate SSEConv.  side_out: f32 [n][vox][2] (optional).  level_map: f32
 * [n][vox] head pre-activation map (optional): += head_w[k]*drop[n][k]*side[k] (SE_UNet.py:232-233). */
int seunet_gate_epilogue_fwd(int dtype, const void* raw, const float* mean, const float* rstd, int c, const float* w_se,
                             const float* w_se2, const float* w_side, const float* b_side, float slope, void* e_out,
                             float* side_out, float* level_map, int level_accumulate, const float* head_w,
                             const float* drop, int drop_stride, seunet_dims dims, seunet_stream_t s);
/* backward, two recompute passes (dxhat itself is never stored; the loss gradient has a large common-mode
 * part that the InstanceNorm backward cancels, so the per-(n,c) sums are taken in f64 and the centred
 * result is rounded exactly once):
 *   pass A (m1 == NULL): stat_partial f64 [n][slots][c][2] = sums of dxhat, dxhat*xhat; pgrad_partial f32
 *                        [n*slots][4c+4] = dw_se | dw_se2 | dw_side[2][c] | db_side[2] | dhead_w[2]
 *   seunet_stats_finalize(mode 1) -> m1, m2 ; seunet_pgrad_reduce -> parameter gradients
 *   pass B (m1, m2 given): draw_out = rstd*(dxhat - m1 - xhat*m2), gradient w.r.t. the raw conv output
 *                          (may alias g_e). */
int seunet_gate_epilogue_bwd(int dtype, const void* raw, const float* mean, const float* rstd, int c, const float* w_se,
                             const float* w_se2, const float* w_side, const float* b_side, float slope, const void* g_e,
                             const float* g_side, const float* g_level, const float* head_w, const float* drop,
                             int drop_stride, const float* m1, const float* m2, void* draw_out, double* stat_partial,
                             float* pgrad_partial, seunet_dims dims, seunet_stream_t s);
int seunet_pgrad_reduce(const float* pgrad_partial, int records, int c, float* dw_se, float* dw_se2, float* dw_side,
                        float* db_side, float* dhead_w, seunet_stream_t s);
/* What the network runs between pass A and pass B, in one launch: seunet_stats_finalize(mode 1) -> m1, m2 [n][c] and
 * seunet_pgrad_reduce over the block records.  Preconditions (checked): c a power of two in [8, 128]; slots =
 * seunet_epilogue_slots(dims) of the pass-A call and records == n * slots, so that stat_partial holds n * slots * c * 2
 * doubles and pgrad_partial records * (4c + 4) floats.  Any parameter-gradient pointer may be NULL (not written). */
int seunet_gate_bwd_finalize(const double* stat_partial, int slots, int c, int n, long long count, float* m1, float* m2,
                             const float* pgrad_partial, int records, float* dw_se, float* dw_se2, float* dw_side,
                             float* db_side, float* dhead_w, seunet_stream_t s);

/* ---- aggregation block: conv1x1 -> IN -> LeakyReLU (+ x-branch); SE_UNet.py:45-49,187,196,205 -------- */
int seunet_cat_epilogue_fwd(int dtype, const void* raw, const float* mean, const float* rstd, const void* raw2,
                            const float* mean2, const float* rstd2, int c, float slope, void* out, seunet_dims dims,
                            seunet_stream_t s);
/* same two-pass scheme; pass A (m1 == NULL) fills the f64 partials, pass B writes dx (may alias g_out) / dx2 */
int seunet_cat_epilogue_bwd(int dtype, const void* g_out, const void* raw, const float* mean, const float* rstd,
                            const void* raw2, const float* mean2, const float* rstd2, int c, float slope,
                            const float* m1, const float* m2, const float* m1b, const float* m2b, void* dx, void* dx2,
                            double* stat_partial, double* stat_partial2, seunet_dims dims, seunet_stream_t s);

/* Two-branch block whose second branch is the 1x1x1 conv of the <= 2-channel network input (x33 / x63 / x93,
 * SE_UNet.py:112,118,124,187,196,205).  That conv's output is never materialised: every pass recomputes
 * raw2[c] = w2[c][0]*x0 + w2[c][1]*x1 from x_in, the packed 8-channel input [N][D][H][W][8] of the level (16 B per voxel
 * instead of 2*c); its InstanceNorm statistics follow from the input's second moments (seunet_xbranch_moments ->
 * seunet_xbranch_stats, exact in f64; moments_out, optional, keeps the per-sample means of x0, x1, x0^2, x0 x1, x1^2 for
 * the backward pass).  The conv's weight gradient dW2[c][i] = sum_v draw2[c] * x[i] is what is left of O(1) terms that cancel
 * to ~1e-5 of their size at 128^3, so it is not accumulated from the f32 draw2: pass A of the backward also sums
 * dxhat2[c] * x[i] (one f64 record per block in xw_partial: n * seunet_epilogue_slots(dims) * c * 2 doubles) and
 * seunet_cat_xgrad_finalize forms dw (c, in_channel, 1, 1, 1) in f64 from those sums, stat_partial2 and the moments
 * (train.py:602 loss.backward() through SE_UNet.py:112,118,124).  w2: (c, in_channel) f32. */
int seunet_xbranch_moment_slots(seunet_dims dims);
int seunet_xbranch_moments(int dtype, const void* x_in, double* partial /* [n][slots][5] */, seunet_dims dims, seunet_stream_t s);
int seunet_xbranch_stats(const double* partial, int slots, const float* w2, int c, int in_channel, int n, long long count,
                         float eps, float* mean2, float* rstd2, double* moments_out /* [n][5] or NULL */, seunet_stream_t s);
int seunet_cat_epilogue_fwd_x(int dtype, const void* raw, const float* mean, const float* rstd, const void* x_in,
                              const float* w2, int in_channel, const float* mean2, const float* rstd2, int c, float slope,
                              void* out, seunet_dims dims, seunet_stream_t s);
/* pass A (m1 == NULL): f64 partials of both branches (+ xw_partial when given); pass B: dx (may alias g_out) */
int seunet_cat_epilogue_bwd_x(int dtype, const void* g_out, const void* raw, const float* mean, const float* rstd,
                              const void* x_in, const float* w2, int in_channel, const float* mean2, const float* rstd2,
                              int c, float slope, const float* m1, const float* m2, const float* m1b, const float* m2b,
                              void* dx, double* stat_partial, double* stat_partial2, double* xw_partial, seunet_dims dims,
                              seunet_stream_t s);
/* The same block followed by nn.MaxPool3d(2,2) (ec33 -> pool0, ec63 -> pool1, ec93 -> pool2; even extents), as the network
 * runs it: one kernel writes out, pooled [n][d/2][h/2][w/2][c] and, when argmax is not NULL, one 32-bit word per pooling
 * window and group of 8 channels, argmax [n][vox/8][c/8]: bits [3j, 3j+3) of word (window, g) hold, for channel 8g + j, the
 * position k = 4*(z&1) + 2*(y&1) + (x&1) of the FIRST maximum, in that z-y-x order, of the window's values AS STORED in out
 * (bits 24-31 are zero).  The backward takes the pooled gradient pool_g [n][vox/8][c] (storage type) with those words and
 * adds it on the fly, in both passes, to g_out at the voxel each word names; pool_argmax == NULL is seunet_cat_epilogue_bwd_x. */
int seunet_cat_epilogue_fwd_x_pool(int dtype, const void* raw, const float* mean, const float* rstd, const void* x_in,
                                   const float* w2, int in_channel, const float* mean2, const float* rstd2, int c, float slope,
                                   void* out, void* pooled, unsigned int* argmax, seunet_dims dims, seunet_stream_t s);
int seunet_cat_epilogue_bwd_x_pool(int dtype, const void* g_out, const void* raw, const float* mean, const float* rstd,
                                   const void* x_in, const float* w2, int in_channel, const float* mean2, const float* rstd2,
                                   int c, float slope, const float* m1, const float* m2, const float* m1b, const float* m2b,
                                   void* dx, double* stat_partial, double* stat_partial2, double* xw_partial,
                                   const unsigned int* pool_argmax, const void* pool_g, seunet_dims dims, seunet_stream_t s);
int seunet_cat_xgrad_finalize(const double* xw_partial, const double* stat_partial2, int slots, const double* moments,
                              const float* w2, int c, int in_channel, int n, float eps, float* dw, seunet_stream_t s);

/* ---- nn.MaxPool3d(2,2) SE_UNet.py:131-133 ; nn.Upsample(x2 trilinear align_corners) :136-138 ---------- */
int seunet_maxpool_fwd(int dtype, const void* in, int c, void* out, seunet_dims in_dims, seunet_stream_t s);
int seunet_maxpool_bwd(int dtype, const void* in, const void* g_out, int c, void* g_in, int accumulate,
                       seunet_dims in_dims, seunet_stream_t s);
int seunet_upsample2_fwd(int dtype, const void* in, int c, void* out, seunet_dims in_dims, seunet_stream_t s);
int seunet_upsample2_bwd(int dtype, const void* g_out, int c, void* g_in, int accumulate, seunet_dims in_dims,
                         seunet_stream_t s);
/* side map [n][vox_low][c] f32 -> NCDHW f32 channels [c_off, c_off+c) of an (n, c_total, ...) tensor */
int seunet_side_upsample(const float* side, int c, int scale, float* out_ncdhw, int c_total, int c_off,
                         seunet_dims low_dims, seunet_stream_t s);

/* ---- heads: dc0_0 / dc0_1 over the DropLayer-scaled side stack; SE_UNet.py:150-153,232-233 ------------
 * level l has extents (D >> l, H >> l, W >> l): D, H and W must be multiples of 2^(nlevels - 1) (W of 4 as well);
 * other extents are refused with an error and nothing is launched. */
int seunet_head_fwd(const float* const* level_maps, int nlevels, const float* bias, float* pred, seunet_dims dims,
                    seunet_stream_t s);
size_t seunet_head_bwd_tmp_floats(seunet_dims dims);
int seunet_head_bwd(const float* g_pred, float* const* g_levels, int nlevels, float* tmp, float* g_bias,
                    seunet_dims dims, seunet_stream_t s);

/* ---- losses: dice_loss / general_union_loss_lib / atr_loss; train.py:51-76 ------------------------------
 * sums[7] (f64, device): see csrc/loss.hip.  The caller forms the loss from the sums (and all-reduces
 * them first under data parallelism), then calls seunet_loss_grad; the upstream gradient is
 * g_scale * (g_scale_dev ? *g_scale_dev : 1) so it can stay on the device.
 * terms: which losses the caller will form (SEUNET_LOSS_DICE | SEUNET_LOSS_GUL | SEUNET_LOSS_ATR; 0 = all): the sums of the
 * others are left 0 (the general-union term's pow is the expensive part of the pass; a Dice-only step skips it). */
#define SEUNET_LOSS_DICE 1
#define SEUNET_LOSS_GUL 2
#define SEUNET_LOSS_ATR 4
int seunet_loss_partial_floats(void);
int seunet_loss_sums(const float* pred, int apply_sigmoid, const float* target, const float* weight, const float* skel,
                     long long n, float* partial, double* sums, int terms, seunet_stream_t s);
/* loss value of one head (sums1 == NULL) or of a training stage's two heads from their sums, on the device:
 * f32(c_dice*dice + c_gul*gul + c_atr*atr of sums0) + f32(the same of sums1), each formed in f64 (the scalar arithmetic of
 * train.py:51-76 and the stage sums train.py:597-599,433-435,241-243 without a dozen one-element kernels). */
int seunet_loss_value(const double* sums0, double c_dice0, double c_gul0, double c_atr0, const double* sums1, double c_dice1,
                      double c_gul1, double c_atr1, float* value, seunet_stream_t s);
int seunet_loss_grad(const float* pred, int apply_sigmoid, const float* target, const float* weight, const float* skel,
                     long long n, const double* sums, float c_dice, float c_gul, float c_atr, float g_scale,
                     const float* g_scale_dev, float* g_pred, seunet_stream_t s);

/* Per-sample sums and values: the key of the online hard mining, train.py:442-446 and :249-253 (one
 * general_union_loss_lib(pred_de[i], label[i], weight[i]).item() per sample there; here one pass and no synchronise).
 * Sample b covers elements [b n, (b + 1) n) of every tensor; sums: [batch][7] f64 as above, values: [batch] f32, each
 * f32(c_dice*dice + c_gul*gul + c_atr*atr) of that sample's sums formed in f64.  partial: seunet_loss_sample_partial_floats
 * (batch) floats of scratch.  A sample's sums are the same bits whatever the batch it is part of and whatever `terms`
 * asks for beside them.  batch <= 65535. */
int seunet_loss_sample_partial_floats(int batch);
int seunet_loss_sums_per_sample(const float* pred, int apply_sigmoid, const float* target, const float* weight, const float* skel,
                                int batch, long long n_per_sample, float* partial, double* sums, int terms, seunet_stream_t s);
int seunet_loss_sample_values(const double* sums, int batch, double c_dice, double c_gul, double c_atr, float* values,
                              seunet_stream_t s);

/* ---- soft skeleton, soft clDice loss (Shit et al., CVPR 2021) and the hard clDice counts (csrc/cldice.hip; the definition
 * is tests/cldice_oracle.py) ------------------------------------------------------------------------------------------------
 * Tensors are `volumes` independent (n0, n1, n2) float32 volumes back to back; pooling never crosses from one into the next.
 * iters: 0 .. 16.  Every call orders all of its work on s and none synchronises the host.
 *   seunet_soft_skeleton: out = S_iters of x, bit for bit the float32 oracle's.  save != 0 also fills the workspace with what
 *     seunet_cldice_backward reads (the workspace then belongs to that pair of calls; the backward leaves the saved state as
 *     it is, so it can run again).  workspace: seunet_cldice_workspace_bytes with the same arguments (host only; 0 + error
 *     for an empty shape or bad iters).
 *   seunet_cldice_sums: sums[4] (f64) = sum S(p) t, sum S(p), sum S(t) p, sum S(t) over n voxels, formed in float64 in a fixed
 *     order; partial: seunet_cldice_partial_doubles() doubles of scratch.  Under data parallelism the caller all-reduces the
 *     four sums before the next two calls.
 *   seunet_cldice_value: value[0] = f32(1 - 2 tprec tsens / (tprec + tsens)), tprec = (sums[0] + smooth) / (sums[1] + smooth),
 *     tsens = (sums[2] + smooth) / (sums[3] + smooth); scalars (optional, f64[2]) = dL/dtprec, dL/dtsens.
 *   seunet_cldice_backward: grad = g_dev[0] * dL/dpred for the prediction whose saving forward filled `workspace`, by the
 *     recorded arg-min / arg-max choices, in gather form (no float atomics: the same bits every run).
 *   seunet_cldice_counts: counts[4] (u64) = |S_P and V_L|, |S_P|, |S_L and V_P|, |S_L| of four uint8 masks (non-zero = 1). */
size_t seunet_cldice_workspace_bytes(long long volumes, int n0, int n1, int n2, int iters, int save);
int seunet_cldice_partial_doubles(void);
int seunet_soft_skeleton(const float* x, long long volumes, int n0, int n1, int n2, int iters, float* out, int save, void* workspace,
                         size_t workspace_bytes, seunet_stream_t s);
int seunet_cldice_sums(const float* skel_pred, const float* target, const float* skel_target, const float* pred, long long n,
                       double* partial, double* sums, seunet_stream_t s);
int seunet_cldice_value(const double* sums, double smooth, float* value, double* scalars, seunet_stream_t s);
int seunet_cldice_backward(const float* target, const float* skel_target, const double* sums, double smooth, const float* g_dev,
                           long long volumes, int n0, int n1, int n2, int iters, float* grad, void* workspace, size_t workspace_bytes,
                           seunet_stream_t s);
int seunet_cldice_counts(const unsigned char* skel_pred, const unsigned char* label, const unsigned char* skel_label,
                         const unsigned char* pred, long long n, unsigned long long* counts, seunet_stream_t s);

/* ---- online hard mining: the sample pool of save_data_online / save_data_online3 (train.py:78-138) and OnlineHMData /
 * OnlineHMData3 (data.py:586-630) in HBM ----------------------------------------------------------------------------------
 * The pool keeps the `capacity` samples with the largest key.  All of it is caller-owned device memory:
 *   pool_data (K, 2, V) f32, pool_weight (K, 1, V) f32, pool_label / pool_skel (K, 1, V) u8 (pool_skel optional),
 *   keys (K) f32, seq (K) i64, state (2) i64 = {count, next sequence number}; zeroing `state` empties the pool.
 * V = voxels per sample, V % 16 == 0; every tensor 16-byte aligned; K = capacity <= 65535.
 *   select:  one small launch; walks new_keys[0..batch) in order like the loop of save_data_online and writes slots_out
 *            (DEVICE, [batch]): the slot a sample is stored in, or -1.  A non-finite key is never stored.  While the pool is
 *            not full the next free slot is taken.  A full pool gives up its minimum (key, seq) entry -- of equal keys the
 *            oldest -- unless the new key is strictly smaller (bisect.bisect, train.py:94-95: a key equal to the minimum is
 *            accepted).  When a later sample of the call takes the slot an earlier one of the same call was given, the earlier
 *            entry of slots_out becomes -1, so the slots of a call are distinct.  batch <= 1024.
 *   scatter: one launch, the batch's data (batch, 2, V) / label / weight / skel (batch, 1, V) f32 into the slots of slots_dev
 *            (DEVICE; negative or >= capacity: that sample is skipped).  label and skel must hold 0.0 and 1.0 only; they are
 *            stored as (unsigned char)v.  data and weight are stored bit for bit.
 *   gather:  slots_host is a HOST array (n <= 32, like `starts` of seunet_crop_batch); writes data_out (n, 2, V) and
 *            label_out / weight_out / skel_out (n, 1, V) f32, the tensors train.py:479-481 builds. */
int seunet_pool_select(const float* new_keys, int batch, float* keys, long long* seq, long long* state, int capacity, int* slots_out,
                       seunet_stream_t s);
int seunet_pool_scatter(const int* slots_dev, int batch, int capacity, long long voxels, const float* data, const float* label,
                        const float* weight, const float* skel, float* pool_data, unsigned char* pool_label, float* pool_weight,
                        unsigned char* pool_skel, seunet_stream_t s);
int seunet_pool_gather(const int* slots_host, int n, int capacity, long long voxels, const float* pool_data,
                       const unsigned char* pool_label, const float* pool_weight, const unsigned char* pool_skel, float* data_out,
                       float* label_out, float* weight_out, float* skel_out, seunet_stream_t s);

/* ---- optimizer step: torch.optim.AdamW(model.parameters(), lr=0.0001).step() -----------------
 * Replaces optimizer.step() at train.py:247,439,603 (constructed at train.py:188,386,569 with PyTorch's default
 * betas=(0.9,0.999), eps=1e-8, weight_decay=0.01, amsgrad=False).  All n tensors of a step are updated by
 * ceil(n/24) launches; pointer arrays are HOST arrays of DEVICE pointers to contiguous f32 tensors of counts[i]
 * elements.  `step` counts from 1 (the value of state['step'] AFTER the increment).  lr is passed per call, so
 * torch.optim.lr_scheduler.MultiStepLR (train.py:189-191) keeps working on the host side.  Hyper-parameters are
 * doubles because PyTorch forms 1-beta, 1-lr*wd and the bias corrections in double before rounding to f32. */
int seunet_adamw_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                      const long long* counts, int n_tensors, double lr, double beta1, double beta2, double eps,
                      double weight_decay, int step, int maximize, seunet_stream_t s);
/* The same step behind a device flag: when *skip_flag (a DEVICE int, written earlier on the stream by a backward pass whose
 * scaled fp16 gradients overflowed) is non-zero, parameters and both moments keep their bits and every tensor's device count
 * skipped[i] (one f32 holding a whole number) grows by one; otherwise the step is applied with the bias corrections of the
 * tensor's EFFECTIVE step steps[i] - *skipped[i] (steps: HOST array, state['step'] after the increment).  Nothing is read on
 * the host.  table: DEVICE scratch of 2 * n_tensors floats, fully written before it is read (prior contents do not matter).
 * The flag is only read: the caller clears it on the stream after the last call of an optimizer step. */
int seunet_adamw_step_gated(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                            const long long* counts, const int* steps, float* const* skipped, int n_tensors, double lr,
                            double beta1, double beta2, double eps, double weight_decay, int maximize, const int* skip_flag,
                            float* table, seunet_stream_t s);

/* ---- input pipeline: one resident case -> the tensors of a training step, in one launch ------------------
 * Replaces, for a mini-batch of crops: crop extraction (data.py:645-664, :85-252), the two HU windows (data.py:667-677,
 * :286-299, :775-784 = prediction.py:39-49), (mask > 0) (data.py:675), weight ** (U + 2) * label + (1 - label)
 * (data.py:701, :389, :561) and the flip / rotate augmentation (data.py:40-67), and writes the layout train.py:582-592
 * builds: data_out (ncrop, 2, cube^3) [2048-window, 1500-window], label_out / weight_out / skel_out (ncrop, 1, cube^3), f32.
 * img: (d, h, w) HU (= file value - 1024, data.py:692), int16 or float32; label / skeleton: uint8 or NULL; weight: float16
 * (the LIB maps, lib_weight.py:50) / float32 / float64 or NULL.  starts: HOST (z, y, x) per crop; aug: HOST code per crop
 * (NULL = none): bit k = source axis k reversed, bit 3 = source axes 1 and 2 fed by output axes 2 and 1 (random_flip then
 * random_rotate composed; all random draws stay with the caller).  weight_exponent = U + 2.  f64_math: 1 = true division
 * in float64 then one rounding (int crops, data.py:286-299; prediction.py:40), 0 = float32 division (data.py:667-677).
 * cube % 32 == 0, ncrop <= 32 per call. */
#define SEUNET_IMG_I16 0
#define SEUNET_IMG_F32 1
#define SEUNET_W_F16 0
#define SEUNET_W_F32 1
#define SEUNET_W_F64 2
int seunet_crop_batch(const void* img, int img_dtype, const unsigned char* label, const void* weight, int weight_dtype,
                      const unsigned char* skeleton, int d, int h, int w, int cube, int ncrop, const int* starts, const int* aug,
                      double weight_exponent, int f64_math, float* data_out, float* label_out, float* weight_out, float* skel_out,
                      seunet_stream_t s);
/* whole-volume network input of the inference / validation loops (prediction.py:39-49,71-75; data.py:775-784,796-798):
 * out (2, nvox) f32 = [2048-window | 1500-window] */
int seunet_hu_two_channel(const void* img, int img_dtype, long long nvox, int f64_math, float* out, seunet_stream_t s);

/* ---- sliding-window assembly: the data movement of prediction.py:78-109 and of the validation /
 * test loops train.py:682-691, test.py:151-161 (window table: data.py:731-773), on the device.
 * volume: (c, x, y, z) f32 NCDHW of ONE case, resident in HBM (prediction.py:77 `x.cuda()`); starts: HOST array of
 * nwin (xl, yl, zl) triples, nwin <= 64 per call; windows are cube^3 (cube % 4 == 0).
 *   gather:      out (nwin, c, cube, cube, cube) f32 = volume[:, xl:xl+cube, yl:yl+cube, zl:zl+cube]   (prediction.py:102)
 *   accumulate:  acc[xl:.., yl:.., zl:..] += sigmoid(logits[k]) in float64, k in list order, no atomics   (:104-106)
 *   finalize:    out = acc / pred_num, pred_num rebuilt from the per-axis window starts (the windows are a product
 *                grid) plus dup0 extra copies of window 0 = (xs[0], ys[0], zs[0]) (data.py:764-765)          (:107,109) */
int seunet_window_gather(const float* volume, int c, int x, int y, int z, int cube, int nwin, const int* starts, float* out,
                         seunet_stream_t s);
int seunet_window_accumulate(const float* logits, int apply_sigmoid, int nwin, const int* starts, int cube, double* acc, int x, int y,
                             int z, seunet_stream_t s);
int seunet_window_finalize(const double* acc, int x, int y, int z, int cube, int nx, const int* xs, int ny, const int* ys, int nz,
                           const int* zs, int dup0, double* out, seunet_stream_t s);

/* ---- post-processing: double_threshold_iteration ----------------------------------------------
 * The reference carries three copies that differ in one line: prediction.py:13-37 keeps pred*255 in float64 (:19);
 * train.py:25-49 and test.py:18-42 (validation / test) round it to float32 (train.py:31, test.py:24), so values within
 * a float32 ulp of a threshold classify differently.  pred_dtype selects the copy: SEUNET_DTI_F64 | SEUNET_DTI_F32.
 * pred: (h, w, z) float64 probabilities on the device (the overlap-averaged volume, prediction.py:109, train.py:693);
 * out: h*w*z bytes, 1 where the reference's result is 1.0.  Reproduces the reference's single in-place raster-order
 * sweep bit for bit.  workspace: seunet_dti_workspace_bytes(h, w, z) bytes, caller-owned. */
#define SEUNET_DTI_F64 0
#define SEUNET_DTI_F32 1
size_t seunet_dti_workspace_bytes(int h, int w, int z);
int seunet_dti(const double* pred, int h, int w, int z, double h_thresh, double l_thresh, int pred_dtype, unsigned char* out,
               void* workspace, size_t workspace_bytes, seunet_stream_t s);

/* ---- largest component, hole filling, metric sums -------------------------------------------------------
 * seunet_largest_component: volume (h, w, z) bytes, non-zero = foreground (the thresholded prediction, prediction.py:110-116).
 *   rule SEUNET_CC_EVALUATION (train.py:749-757): out = the 26-connected component with the most voxels (ties: the one that
 *        appears LAST in raster order = cc3d's highest label, `sorted(..)[::-1]`); an empty volume gives an empty mask.
 *   rule SEUNET_CC_MAXIMUM_3D (util.py:58-75): as above; if that component has no voxel in the slices z//2, z//3, z//3*2 of
 *        the last axis the second component is taken; then scipy.ndimage.binary_fill_holes (6-connected background that
 *        does not reach the border becomes foreground).
 * out: h*w*z bytes of 0/1.  status_dev (device int, optional): 0 ok, 1 no component, 2 no second component (the reference
 * raises IndexError in both cases under maximum_3d).  Union-find with atomics on labels = minimum linear index: the
 * result is deterministic.  workspace: seunet_cc_workspace_bytes(h, w, z), caller-owned.
 *   rule SEUNET_CC_LARGEST_FILLED (util.py:156-165, large_connected_domain26): the component of SEUNET_CC_EVALUATION (ties:
 *        the highest label, as the reference's argsort gives with a stable sort), then the binary_fill_holes of
 *        SEUNET_CC_MAXIMUM_3D; status 1 for an empty volume (the reference raises IndexError). */
#define SEUNET_CC_EVALUATION 0
#define SEUNET_CC_MAXIMUM_3D 1
#define SEUNET_CC_LARGEST_FILLED 2
size_t seunet_cc_workspace_bytes(int h, int w, int z);
int seunet_largest_component(const unsigned char* volume, int h, int w, int z, int rule, unsigned char* out, int* status_dev,
                             void* workspace, size_t workspace_bytes, seunet_stream_t s);
/* The integer sums every ATM'22 metric of metrics.py:14-78 is formed from, in one pass over 0/1 byte volumes pred / label /
 * skeleton and the int32 branch-parsing volume (label, skeleton, parsing optional):
 * out = u64[8] {sum(pred*label), sum(pred), sum(label), sum(pred*skeleton), sum(skeleton), 0, 0, 0}, then u32[nbins] counts of
 * skeleton*parsing (np.bincount, metrics.py:16-17), u32[nbins] counts of skeleton*parsing*pred (:19-21), int max id, int
 * overflow (an id >= nbins was met).  The caller forms the rounded percentages exactly like metrics.py. */
size_t seunet_metric_out_bytes(int nbins);
int seunet_metric_sums(const unsigned char* pred, const unsigned char* label, const unsigned char* skeleton, const int* parsing,
                       long long n, int nbins, void* out, size_t out_bytes, seunet_stream_t s);

/* ---- stage-2/3 preparation: exact EDT, hard-mining candidates, LIB weight, break weight -------------------------------
 * Volumes are C-contiguous (n0, n1, n2) on the device, axis 2 contiguous; masks are bytes with non-zero = 1.  Extents up to
 * 32767 per axis and fewer than 2^31 voxels (anything else: error).  workspaces: the *_workspace_bytes of the same extents.
 *
 * seunet_edt: scipy.ndimage.distance_transform_edt(volume, return_indices=...) with unit sampling: for every voxel the nearest
 *   ZERO voxel.  Outputs (each optional, NULL = skip): sqdist int32 squared distance; dist float64 = the correctly rounded sqrt
 *   (bitwise scipy's); indices int32 (3, n0, n1, n2), the feature transform, bitwise scipy's, ties included.  A volume with no
 *   zero voxel is an error (scipy's values are meaningless there): status_dev (device int, optional) is 1 then, 0 otherwise,
 *   and the outputs are -1.
 * seunet_hard_mining_masks: the candidate lists of data.py:305-306 / :457-458 as bit masks (bit j of word w = voxel 64 w + j in
 *   raster order, ceil(n0 n1 n2 / 64) words each): skeleton_bits = skeleton != 0 and pred != 1 (where(skeleton * (1 - pred)));
 *   small_bits = skeleton == 0 or EDT(label)^2 < 4 (where(dis * skeleton < 2)).  seunet_mask_bits packs any mask the same way
 *   (loc_break = where(br_skel == 1)).
 * seunet_lib_weight: lib_weight.py:36-53 (save_lib_weight, no ** 2.5): out = float16 (raw 16-bit) table[c] * label, c the 7x7x7
 *   count of label voxels with mode 'mirror'; table: 344 host floats, table[k] = -log10(float32(k) / 343), table[0] = -log10(1).
 * seunet_break_weight: weight_br.py:113-177 (save_weight_break) with the skeleton given: w_br float16 (raw 16-bit) and br_skel
 *   bytes.  When the reference's maxf is 0 both are all zeros.  An empty skeleton is an error (status_dev 1). */
size_t seunet_edt_workspace_bytes(int n0, int n1, int n2);
int seunet_edt(const unsigned char* volume, int n0, int n1, int n2, int* sqdist, double* dist, int* indices, int* status_dev,
               void* workspace, size_t workspace_bytes, seunet_stream_t s);
/* seunet_edt_sampling: scipy.ndimage.distance_transform_edt(volume, sampling=(s0, s1, s2), return_indices=True): the nearest ZERO
 *   voxel of every voxel when voxel (i0, i1, i2) lies at (i0 s0, i1 s1, i2 s2).  scipy's feature transform in float64, operation
 *   by operation with no fused multiply-add; s0, s1, s2 positive and finite (anything else: error), passed
 *   by value.  Outputs (each optional, NULL = skip): dist float64 = sqrt((dt_0^2 + dt_1^2) + dt_2^2) with
 *   dt_a = (double)(index_a - coordinate_a) * s_a, bitwise scipy's; indices int32 (3, n0, n1, n2), bitwise scipy's, ties included;
 *   lin int32, the linear index (i0 n1 + i1) n2 + i2 of the feature.  status_dev and a volume with no zero voxel: as seunet_edt.
 *   All work is ordered on s; the call does not synchronise.  workspace: seunet_edt_sampling_workspace_bytes (8 bytes per voxel). */
size_t seunet_edt_sampling_workspace_bytes(int n0, int n1, int n2);
int seunet_edt_sampling(const unsigned char* volume, int n0, int n1, int n2, double s0, double s1, double s2, double* dist, int* indices,
                        int* lin, int* status_dev, void* workspace, size_t workspace_bytes, seunet_stream_t s);
int seunet_mask_bits(const unsigned char* mask, long long n, unsigned long long* bits, seunet_stream_t s);
int seunet_hard_mining_masks(const unsigned char* label, const unsigned char* skeleton, const unsigned char* pred, int n0, int n1,
                             int n2, unsigned long long* skeleton_bits, unsigned long long* small_bits, seunet_stream_t s);
size_t seunet_lib_weight_workspace_bytes(int n0, int n1, int n2);
int seunet_lib_weight(const unsigned char* label, int n0, int n1, int n2, const float* table, void* out, void* workspace,
                      size_t workspace_bytes, seunet_stream_t s);
size_t seunet_break_weight_workspace_bytes(int n0, int n1, int n2);
int seunet_break_weight(const unsigned char* label, const unsigned char* pred, const unsigned char* skeleton, int n0, int n1, int n2,
                        void* w_br, unsigned char* br_skel, int* status_dev, void* workspace, size_t workspace_bytes,
                        seunet_stream_t s);

/* ---- 3-D skeletonisation ------------------------------------------------------------------------
 * seunet_skeletonize: volume (n0, n1, n2) bytes, C-contiguous on the device, non-zero = foreground; out: n0*n1*n2 bytes, 1 on
 * the skeleton and 0 elsewhere (out may not alias volume; the input is not modified).  The reference takes this volume from
 * skimage.morphology.skeletonize_3d on the CPU (ske_and_parse.py:83, weight_br.py:128, prediction.py:127).  Here: Lee, Kashyap
 * and Chu (1994) with the border order and raster-order re-check of the common implementations; equality with skimage has not
 * been checked.  The definition is DESIGN.md 3d and tests/skeleton_oracle.py, which the result equals bit for bit; it is
 * deterministic.  Any extents >= 1 with at most 2^31-1 voxels and fewer than 2^32 64-voxel words after padding (anything else:
 * error).  passes_dev (device int, optional): the number of passes run, the last one, which deletes nothing, included.
 * The call synchronises the stream once per pass.  workspace: seunet_skeleton_workspace_bytes(n0, n1, n2), caller-owned
 * (0 and a message in seunet_last_error for extents outside the range above). */
size_t seunet_skeleton_workspace_bytes(int n0, int n1, int n2);
int seunet_skeletonize(const unsigned char* volume, int n0, int n1, int n2, unsigned char* out, int* passes_dev, void* workspace,
                       size_t workspace_bytes, seunet_stream_t s);

/* ---- airway tree parsing: the ATM'22 branch labelling --------------------------------------------
 * atm22_skel_parse.py:83-135 as driven by tree_parsing.py:114-159.  Volumes are C-contiguous (n0, n1, n2) on the device, axis 2
 * contiguous; masks are bytes with non-zero = 1; label volumes are int32.  Fewer than 2^31 voxels; seunet_parse_assign also has
 * the EDT's limit of 32767 per axis (anything else: error).  Integer work throughout: every output is bitwise the reference's
 * and does not depend on the order in which the device executes anything.  workspaces: the *_workspace_bytes of the same
 * extents, caller-owned; nothing is allocated and no call synchronises the stream (num_dev / status_dev are device ints the
 * caller reads when it needs them on the host).
 *
 * seunet_skeleton_branches: skeleton_parsing (:83-101).  A skeleton voxel whose 3x3x3 sum with mode 'reflect' (index -1 -> 0,
 *   n -> n - 1: a voxel on a face counts itself and its in-face neighbours again) exceeds 3 is a branch point and is removed;
 *   the rest is labelled with 26-connectivity; components with fewer than min_voxels voxels (the reference: 5) are removed; the
 *   survivors are numbered 1..num in raster order of their first voxel, as the reference's second ndimage.label numbers them.
 *   cd: int32 numbers (0 elsewhere); skeleton_parse (optional): bytes, cd != 0; num_dev (device int, optional): num.
 * seunet_parse_assign: tree_parsing_func (:103-108): parsing[v] = label[v] != 0 ? cd[f(v)] : 0 with f(v) the feature transform
 *   of seunet_edt (bitwise scipy's, ties included) for the sites skeleton_parse != 0.  The (3, n0, n1, n2) index volume is
 *   never stored: the last EDT pass gathers cd.  An empty skeleton_parse is an error: status_dev (device int, optional) is 1
 *   then, 0 otherwise, and parsing is all zeros.
 * seunet_label_stats: the statistics loc_trachea and adjacent_map (:110-135) take from a label volume with values 0..num:
 *   counts = device u32[num + 1] voxels per value; adjacency_bits = (num + 1) rows of ceil((num + 1) / 64) u64 words, bit b of
 *   word w of row a set iff values a != 64 w + b, both > 0, meet across a face (symmetric).  Both are zeroed here.  status_dev
 *   (device int): 1 if a value outside 0..num was met (it is ignored), 0 otherwise.  num <= seunet_label_stats_max_num() = 4095
 *   (the default nbins of the metric sums - 1): a larger num is an error.
 * seunet_relabel: out[i] = lut[parsing[i]] over n elements, lut = device int32[nlut]; a value outside 0..nlut-1 gives 0.  out may
 *   alias parsing. */
size_t seunet_skeleton_branches_workspace_bytes(int n0, int n1, int n2);
int seunet_skeleton_branches(const unsigned char* skeleton, int n0, int n1, int n2, int min_voxels, int* cd, unsigned char* skeleton_parse,
                             int* num_dev, void* workspace, size_t workspace_bytes, seunet_stream_t s);
size_t seunet_parse_assign_workspace_bytes(int n0, int n1, int n2);
int seunet_parse_assign(const unsigned char* skeleton_parse, const int* cd, const unsigned char* label, int n0, int n1, int n2,
                        int* parsing, int* status_dev, void* workspace, size_t workspace_bytes, seunet_stream_t s);
int seunet_label_stats_max_num(void);
int seunet_label_stats(const int* parsing, int n0, int n1, int n2, int num, unsigned int* counts, unsigned long long* adjacency_bits,
                       int* status_dev, seunet_stream_t s);
int seunet_relabel(const int* parsing, long long n, const int* lut, int nlut, int* out, seunet_stream_t s);

/* ---- airway tree parsing: the reference's own parser -----------------------------------------------
 * What ske_and_parse.py:20-65 (airway_parse) with ours_skel_parse.py:569-619 (Topology_Tree.sub / merge) needs from the device
 * besides seunet_largest_component, seunet_skeletonize, seunet_mask_bits, seunet_mask_box, seunet_crop3d and seunet_parse_assign;
 * its graph stage runs on the host.  Volumes are C-contiguous (n0, n1, n2) on the device, axis 2 contiguous; masks are bytes
 * with non-zero = 1; fewer than 2^31 voxels (anything else: error).  Integer work throughout: every output is bitwise scipy's and
 * does not depend on the order in which the device executes anything.  Nothing is allocated and no call synchronises the stream.
 *
 * seunet_binary_morph: skimage.morphology.binary_dilation / binary_closing with the default footprint, the cross of the 6 face
 *   neighbours, as scipy.ndimage states them (not checked against skimage): SEUNET_MORPH_DILATE, outside the volume = 0;
 *   SEUNET_MORPH_ERODE_BORDER0 / _BORDER1, outside = 0 / 1 (binary_erosion(border_value=...)); SEUNET_MORPH_CLOSE = DILATE then
 *   ERODE_BORDER1, bit for bit.  out: n0*n1*n2 bytes of 0/1, may not alias volume.  workspace:
 *   seunet_binary_morph_workspace_bytes(n0, n1, n2), caller-owned (two bit-packed copies of the volume).
 * seunet_fill_holes: scipy.ndimage.binary_fill_holes: out = volume != 0, plus the 6-connected background that does not reach
 *   the border of the volume: the hole-filling stage of seunet_largest_component on its own.  out: bytes of 0/1, may alias
 *   volume.  workspace: seunet_cc_workspace_bytes(n0, n1, n2).
 * seunet_slice_moments: out_dev = 3 device u64 {count, sum of i0, sum of i1} over the non-zero voxels of the slice [:, :, k]
 *   (zeroed here): the exact sums behind the centroids of compute_base_vector (ours_skel_parse.py:178-183).
 * seunet_scatter_labels: cd[lin_index[j]] = value[j] and skeleton_parse[lin_index[j]] = (value[j] != 0) for j < m, into volumes
 *   of n voxels the caller has zeroed (ske_and_parse.py:48-62); lin_index = device int64 raster indices, value = device int32.
 *   The caller passes every voxel once (the first writer is resolved on the host), so the device order decides nothing.  An
 *   index outside 0..n-1 is skipped and sets status_dev (device int, zeroed here) to 1. */
#define SEUNET_MORPH_DILATE 0
#define SEUNET_MORPH_ERODE_BORDER0 1
#define SEUNET_MORPH_ERODE_BORDER1 2
#define SEUNET_MORPH_CLOSE 3
size_t seunet_binary_morph_workspace_bytes(int n0, int n1, int n2);
int seunet_binary_morph(const unsigned char* volume, int n0, int n1, int n2, int op, unsigned char* out, void* workspace,
                        size_t workspace_bytes, seunet_stream_t s);
int seunet_fill_holes(const unsigned char* volume, int n0, int n1, int n2, unsigned char* out, void* workspace, size_t workspace_bytes,
                      seunet_stream_t s);
int seunet_slice_moments(const unsigned char* mask, int n0, int n1, int n2, int k, unsigned long long* out_dev, seunet_stream_t s);
int seunet_scatter_labels(const long long* lin_index_dev, const int* value_dev, long long m, long long n, int* cd,
                          unsigned char* skeleton_parse, int* status_dev, seunet_stream_t s);

/* ---- surface meshing: prediction.py:121-149 ---------------------------------------------------------
 * A 0/1 volume (bytes, non-zero = 1, C-contiguous (n0, n1, n2), fewer than 2^31 voxels) to an indexed triangle mesh, the mesh's
 * vertex adjacency, Jacobi smoothing, the affine step (v - centre) * scale and binary-STL records.  The extraction rule, the
 * vertex and face numbering and the order of every float32 operation are DESIGN.md 3h; every result is deterministic and equals
 * tests/mesh_oracle.py bit for bit.  Equality with skimage's marching_cubes_lewiner or with VTK's smoothing is not claimed.
 * verts are float32 (V, 3), faces int32 (F, 3); V and 3 F beyond the int32 range are an error.
 *
 * seunet_mesh_count: packs the volume, counts and scans; *nverts / *nfaces (HOST) receive V and F.  This call synchronises the
 *   stream once, to read those two numbers; the caller sizes verts and faces with them.  workspace:
 *   seunet_mesh_workspace_bytes(n0, n1, n2), caller-owned, and handed unchanged to seunet_mesh_emit.  A volume with an extent of 1
 *   has no cells and gives V = F = 0.
 * seunet_mesh_emit: writes verts and faces from the workspace seunet_mesh_count left, with the nverts / nfaces it returned;
 *   level strictly between 0 and 1 (the offsets level and 1 - level are formed in double and rounded once to float32).
 * seunet_mesh_coord_sums: sums_dev = 4 device int64 {count, sum of i0, sum of i1, sum of i2} over the non-zero voxels (zeroed
 *   here): the exact sums behind the mean skeleton coordinate the mesh is centred on.
 * seunet_mesh_adjacency: the neighbours of every vertex in CSR form, ascending and without repeats: indptr = nverts + 1 device
 *   int32, indices = room for indices_capacity >= 6 F device int32 of which indptr[nverts] are written, boundary = nverts bytes,
 *   1 where the vertex is an end of a directed face edge whose reverse no face has.  A face with an index outside 0 .. nverts - 1
 *   is left out and sets status_dev (device int, zeroed here) to 1.  6 F beyond the int32 range is an error.  workspace:
 *   seunet_mesh_adjacency_workspace_bytes(nverts, nfaces).
 * seunet_mesh_smooth: n_iter sweeps x' = x + relaxation_factor * (m - x), m = (0 + the neighbours in ascending order) / degree,
 *   per coordinate, one float32 rounding per operation; boundary vertices and vertices without neighbours stay.  indptr, indices,
 *   boundary as seunet_mesh_adjacency wrote them.  out may not alias verts; tmp = a second (nverts, 3) buffer, needed from two
 *   sweeps on.  n_iter = 0 copies.
 * seunet_mesh_affine: out = (verts - centre) * scale per axis in float32; centre, scale = 3 HOST floats each (NULL: 0 / 1).
 *   out may alias verts.
 * seunet_mesh_stl_records: records = 50 F bytes (2-byte aligned): the unit normal of (b - a) x (c - a) (0, 0, 0 for a zero-area
 *   triangle), the three vertices after the affine step, a zero attribute word.  With an 80-byte header and the uint32 F in front
 *   this is a binary STL file.  A face with an index outside 0 .. nverts - 1 gives a zero record and sets status_dev to 1. */
size_t seunet_mesh_workspace_bytes(int n0, int n1, int n2);
int seunet_mesh_count(const unsigned char* volume, int n0, int n1, int n2, long long* nverts, long long* nfaces, void* workspace,
                      size_t workspace_bytes, seunet_stream_t s);
int seunet_mesh_emit(int n0, int n1, int n2, double level, long long nverts, long long nfaces, float* verts, int* faces,
                     const void* workspace, size_t workspace_bytes, seunet_stream_t s);
int seunet_mesh_coord_sums(const unsigned char* mask, int n0, int n1, int n2, long long* sums_dev, seunet_stream_t s);
size_t seunet_mesh_adjacency_workspace_bytes(long long nverts, long long nfaces);
int seunet_mesh_adjacency(const int* faces, long long nfaces, long long nverts, int* indptr, int* indices, long long indices_capacity,
                          unsigned char* boundary, int* status_dev, void* workspace, size_t workspace_bytes, seunet_stream_t s);
int seunet_mesh_smooth(const float* verts, long long nverts, const int* indptr, const int* indices, const unsigned char* boundary,
                       int n_iter, float relaxation_factor, float* out, float* tmp, seunet_stream_t s);
int seunet_mesh_affine(const float* verts, long long nverts, const float* centre, const float* scale, float* out, seunet_stream_t s);
int seunet_mesh_stl_records(const float* verts, long long nverts, const int* faces, long long nfaces, const float* centre,
                            const float* scale, unsigned char* records, int* status_dev, seunet_stream_t s);

/* ---- labelled surface meshing: ours_skel_parse.py:1101-1152, tree_parsing.py:167-196 -----------------
 * An int32 label volume (C-contiguous (n0, n1, n2), values 0 .. num, num <= 65535, fewer than 2^31 voxels) to the meshes of all
 * its labels in one extraction.  The mesh of label k is, bit for bit and index for index, what seunet_mesh_count / seunet_mesh_emit
 * give for the mask "label == k"; the result is their concatenation for k = 1 .. num: verts float32 (V, 3), faces int32 (F, 3)
 * indexing the concatenated verts, and vert_ptr / face_ptr with label k owning verts[vert_ptr[k-1] .. vert_ptr[k]) and
 * faces[face_ptr[k-1] .. face_ptr[k]).  A grid edge between two different non-zero labels carries two vertices, one per label.
 * Every result is deterministic and equals tests/mesh_label_oracle.py.  No launch, pass or synchronisation is per label.
 *
 * seunet_mesh_label_count: checks the labels, counts, scans.  num = the number of labels, or -1 for the largest label present.
 *   *nverts, *nfaces, *num_used, *status (all HOST) receive V, F, the num in force and 0 or a sum of 1 (a negative label) and 2
 *   (a label above num, or above 65535 with num = -1); with a non-zero status the other results mean nothing and
 *   seunet_mesh_label_emit must not follow.  This call synchronises the stream once, to read those four numbers.  vert_ptr_dev,
 *   face_ptr_dev: ptr_capacity device int64 each, ptr_capacity >= num + 1 (65536 with num = -1); entries 0 .. num_used are the
 *   pointers above, left on the device for the caller to read.  workspace: seunet_mesh_label_workspace_bytes(n0, n1, n2),
 *   caller-owned, handed unchanged to seunet_mesh_label_emit.  A volume with an extent of 1 has no cells: V = F = 0, pointers 0.
 * seunet_mesh_label_emit: writes verts and faces with the num_used / nverts / nfaces the count call returned and the same labels
 *   and workspace; level as in seunet_mesh_emit.  The label order comes from a stable radix sort of (label, raster index) in
 *   sort_workspace: seunet_mesh_label_sort_bytes(nverts, nfaces), caller-owned.  V or 3 F beyond the int32 range is an error. */
size_t seunet_mesh_label_workspace_bytes(int n0, int n1, int n2);
size_t seunet_mesh_label_sort_bytes(long long nverts, long long nfaces);
int seunet_mesh_label_count(const int* labels, int n0, int n1, int n2, int num, long long* nverts, long long* nfaces, int* num_used,
                            int* status, long long* vert_ptr_dev, long long* face_ptr_dev, int ptr_capacity, void* workspace,
                            size_t workspace_bytes, seunet_stream_t s);
int seunet_mesh_label_emit(const int* labels, int n0, int n1, int n2, int num, double level, long long nverts, long long nfaces,
                           float* verts, int* faces, const void* workspace, size_t workspace_bytes, void* sort_workspace,
                           size_t sort_bytes, seunet_stream_t s);

/* ---- branch morphometry: the numbers per branch of a labelled airway tree ---------------------------
 * The reference measures nothing per branch; the definition is this comment, restated in numpy by tests/morphometry_oracle.py.
 * parsing: int32 label volume, C-contiguous (n0, n1, n2), values 0 .. num with 0 = background, fewer than 2^31 voxels,
 * num <= seunet_label_stats_max_num() = 4095 (anything else: error).  skeleton: bytes, non-zero = set.  sqdist: the int32 squared
 * distance of seunet_edt, or NULL: r2_sum, r2_min and r2_max keep their empty values then.  A labelled skeleton voxel is one with
 * skeleton != 0 and 1 <= parsing <= num.  Integer work throughout: every output is deterministic and does not depend on the
 * order in which the device executes anything.  No launch, pass or synchronisation is per label; nothing is allocated, no
 * workspace is needed and the call does not synchronise the stream.
 *
 * seunet_branch_stats: device arrays indexed by label value 0 .. num, all written here (row 0 holds the empty values):
 *   voxels int64[num + 1]: voxels with parsing == k.  coord_sum int64[num + 1][3]: the sums of i0, i1, i2 over them.  box_min,
 *   box_max int32[num + 1][3]: their inclusive bounding box; a label without voxels has box_min = (n0, n1, n2), box_max = (-1, -1, -1).
 *   skeleton_voxels int64[num + 1]: labelled skeleton voxels of label k.  links int64[num + 1][13]: counted links whose two ends both
 *   carry label k, by offset class.  cross_links int64[num + 1][13]: counted links with one end of label k and the other end of a
 *   different label >= 1; such a link is counted once in each of the two rows.  r2_sum int64[num + 1], r2_min / r2_max
 *   int32[num + 1]: sum, minimum and maximum of sqdist over the labelled skeleton voxels of k; empty: 0, INT32_MAX, -1.
 *   Links: the 13 offset classes are the offsets d of {-1, 0, 1}^3 lexicographically above (0, 0, 0) in ascending order (class 0 =
 *   (0, 0, 1), class 1 = (0, 1, -1), ..., class 12 = (1, 1, 1)).  A pair (p, p + d) of labelled skeleton voxels inside the volume is
 *   a counted link unless, for some proper non-empty subset of the non-zero components of d, p + (that part of d) is a labelled
 *   skeleton voxel of any label: face links always count, an edge diagonal is dropped when one of its 2 intermediate voxels is
 *   occupied, a corner diagonal when one of its 6 is.
 *   status_dev (device int): 1 if a parsing value outside 0..num was met (that voxel is ignored everywhere), 0 otherwise. */
int seunet_branch_stats(const int* parsing, const unsigned char* skeleton, const int* sqdist, int n0, int n1, int n2, int num,
                        long long* voxels, long long* coord_sum, int* box_min, int* box_max, long long* skeleton_voxels, long long* links,
                        long long* cross_links, long long* r2_sum, int* r2_min, int* r2_max, int* status_dev, seunet_stream_t s);
/* seunet_branch_wall_stats: the distance from the centreline to the wall per label under the voxel spacing (s0, s1, s2), positive
 *   and finite, by value.  indices: int32 (3, n0, n1, n2), the feature transform of seunet_edt_sampling with the same spacing
 *   (-1: no feature).  One streaming pass over skeleton; parsing and indices are read at set skeleton voxels only.  Over the
 *   labelled skeleton voxels of label k that have a feature (device arrays indexed by label value 0 .. num, all written here):
 *   wall_count int64[num + 1]: their number.  offset_sq_sum int64[num + 1][3]: the sums of (index_a - coordinate_a)^2 per axis a.
 *   wall_sq_min / wall_sq_max float64[num + 1]: minimum and maximum of (dt_0^2 + dt_1^2) + dt_2^2 with
 *   dt_a = (double)(index_a - coordinate_a) * s_a, every product and sum rounded on its own; none: +inf and 0.0.
 *   Deterministic: integer sums, and minima / maxima taken on the bit patterns of non-negative doubles.
 *   status_dev (device int): 1 if a skeleton voxel's parsing value is outside 0..num (that voxel is ignored), 0 otherwise. */
int seunet_branch_wall_stats(const int* parsing, const unsigned char* skeleton, const int* indices, int n0, int n1, int n2, int num,
                             double s0, double s1, double s2, long long* wall_count, long long* offset_sq_sum, double* wall_sq_min,
                             double* wall_sq_max, int* status_dev, seunet_stream_t s);

/* ---- airway cross-sections: the lumen section perpendicular to the centreline at every centreline point ---------
 * The reference measures nothing of the kind; the definition is this comment, restated operation by operation in numpy by
 * tests/cross_section_oracle.py, and every output equals that oracle bit for bit.  parsing, skeleton, num: as seunet_branch_stats.
 * A point is a labelled skeleton voxel (skeleton != 0, 1 <= parsing <= num); points are numbered in raster order.
 *
 * seunet_cross_section_count marks and numbers the points (no atomics in the numbering) and synchronises the stream once to
 * return *m, their number, and *status: 1 if a parsing value outside 0..num was met (that voxel is no point), 0 otherwise.
 * workspace: seunet_cross_section_workspace_bytes(n0, n1, n2) bytes, handed unchanged to the emit call.
 *
 * seunet_cross_section_emit (m >= 1, the count call's) writes per point, without synchronising and with no launch or pass per
 * point or per label: lin int32[m], its linear index; tangent float64[m][3]; table int32[m][12] = i0, i1, i2, label, support,
 * count, sum i, sum j, sum i^2, sum j^2, sum ij, rim.  All float64 operations are single IEEE operations in the order written,
 * none contracted into a fused multiply-add.  With p the point, k its label, (s0, s1, s2) the spacing, h = step, W = window (1..7):
 *   tangent  over the skeleton voxels q of label k with |q - p|_inf <= W (p included; support = n, their number), d = q - p:
 *            S_ab = n sum d_a d_b - sum d_a sum d_b in int64; C_ab = ((double)S_ab * s_a) * s_b for a <= b, C_ba = C_ab.  Invalid
 *            (tangent 0, count, moments and rim 0) when n < 3 or max |C_ab| is not positive.  A = C / max |C_ab|; six times
 *            B_ab = (A_a0 A_0b + A_a1 A_1b) + A_a2 A_2b, A = B / max |B_ab|.  The column c of largest (A_0c^2 + A_1c^2) + A_2c^2
 *            (the lowest on a tie) divided by the root of that sum is t; t is negated when its component of largest magnitude
 *            (the lowest on a tie) is negative.
 *   basis    a = the index of smallest |t_a| (the lowest on a tie); w_b = [a == b] - t_a t_b; u = w / sqrt((w_0^2 + w_1^2) + w_2^2);
 *            v = t x u, v_0 = t_1 u_2 - t_2 u_1 and cyclically.
 *   samples  column i and row j in -31..31: x_a = (p_a s_a + (i h) u_a) + (j h) v_a, voxel_a = floor(x_a / s_a + 0.5).  A sample is
 *            inside when its voxel lies in the volume and parsing there equals k (same_label != 0) or is non-zero (same_label == 0).
 *   section  the 4-connected set of inside samples that contains (0, 0); count, the moments and rim (the section's samples with
 *            |i| = 31 or |j| = 31; > 0: the section is cut by the grid) are taken over it.
 * seunet_cross_section_sweep_points: the points one grid sweep of the section pass takes (tests put more points than that). */
size_t seunet_cross_section_workspace_bytes(int n0, int n1, int n2);
int seunet_cross_section_sweep_points(void);
int seunet_cross_section_count(const int* parsing, const unsigned char* skeleton, int n0, int n1, int n2, int num, long long* m, int* status,
                               void* workspace, size_t workspace_bytes, seunet_stream_t s);
int seunet_cross_section_emit(const int* parsing, const unsigned char* skeleton, int n0, int n1, int n2, double s0, double s1, double s2,
                              double step, int window, int same_label, long long m, int* lin, double* tangent, int* table,
                              const void* workspace, size_t workspace_bytes, seunet_stream_t s);

/* ---- airway walls: FWHM wall edges on 64 rays in the section plane of every centreline point ---------------------
 * The reference measures nothing of the kind; the definition is this comment, restated operation by operation in numpy by
 * tests/airway_wall_oracle.py, and every output equals that oracle bit for bit.  All float64 and float32 operations are single
 * IEEE operations in the order written, none contracted into a fused multiply-add.
 *
 * seunet_airway_walls: one launch on stream s, no workspace, no synchronise, no launch or pass per point, per label or per ray.
 * ct: the CT, int16 (ct_dtype = SEUNET_IMG_I16) or finite float32 (SEUNET_IMG_F32), C-contiguous (n0, n1, n2) like parsing (int32
 * labels); a constant shift of the CT (such as +1024) moves an edge by float32 rounding only.  (s0, s1, s2): the spacing; h = step: the section step of
 * the rows; dr = ray_step > 0; n = n_search in 1..31; c = min_contrast > 0 (float32), all finite.  table int32[m][12], tangent
 * float64[m][3]: the rows of seunet_cross_section_emit (i0, i1, i2, label, support, count, sum i, sum j, ..., rim), m >= 1.
 * A point with count == 0 or rim > 0 is not measured: every ray gets code 6, mask 0, sums 0.  Otherwise, with p the point:
 *   frame    u, v from the tangent as in seunet_cross_section_emit's basis.  c_i = (double)sum_i / (double)count, c_j likewise;
 *            the origin is the lumen centroid o_a = (p_a s_a + (c_i h) u_a) + (c_j h) v_a.
 *   rays     r = 0..63 with e_a = C_r u_a + S_r v_a, (C_r, S_r) the committed table of seunet_airway_wall_directions.
 *   samples  k = 0..63 at rho_k = (double)k dr: x_a = o_a + rho_k e_a, g_a = x_a / s_a, f_a = floor(g_a), w_a = (float)(g_a - f_a).
 *            A sample is usable when 0 <= f_a and f_a + 1 <= n_a - 1 on every axis; L = the first unusable k, or 64.  P[k] is the
 *            float32 trilinear value of the CT (corners converted to float32) along axis 2, then 1, then 0, each step
 *            a + w (b - a).  The label g_k is parsing at floor(g_a + 0.5); a sample is inside when g_k == label (same_label != 0)
 *            or g_k != 0 (same_label == 0).
 *   per ray  the first rule that fails gives the code, 0 = measured:
 *            1 no boundary: L == 0, sample 0 not inside, or no k in 1..L-1 that is not inside; k_b = the smallest such k.
 *            2 no peak: k_p = argmax P over max(k_b - 1, 0) .. min(k_b + n, L - 1), the lowest k on a tie; fails when k_p + 1 >= L,
 *              or when k_p is the window's last index and P[k_p + 1] >= P[k_p].
 *            3 no inner contrast: P_l = min P[0..k_p], P_p = P[k_p]; fails when P_p - P_l < c.
 *            4 another lumen: walk k from k_p while k < min(k_p + n, L - 1) and P[k + 1] <= P[k]; k_o = where it stops,
 *              P_o = P[k_o]; fails when g_k != 0 for some k in k_b..k_o.
 *            5 no outer contrast: P_p - P_o < c.
 *            measured: H_in = 0.5f (P_l + P_p); k_i = the largest k < k_p with P[k] <= H_in;
 *              rho_in = ((double)k_i + ((double)H_in - P[k_i]) / ((double)P[k_i + 1] - P[k_i])) dr;
 *              H_out = 0.5f (P_p + P_o); k_e = the smallest k in k_p..k_o - 1 with P[k + 1] <= H_out;
 *              rho_out = ((double)k_e + ((double)P[k_e] - H_out) / ((double)P[k_e] - P[k_e + 1])) dr.
 *            Both denominators are positive: P_l <= H_in < P_p and P_o <= H_out < P_p, because P_p exceeds P_l and P_o by at
 *            least c > 0 (c no smaller than the spacing of float32 at these values, so that the half sum rounds strictly below
 *            P_p); k_i + 1 is then either k_p or an index whose value exceeds H_in >= P[k_i], and P[k_e] is either P_p or a
 *            value above H_out >= P[k_e + 1].  CT magnitudes are below 2^126, so that no difference or sum overflows.
 *   outputs  mask uint64[m]: bit r set when ray r has code 0.  sums float64[m][6]: the sums over the rays of rho_in, rho_out,
 *            rho_in^2, rho_out^2, rho_out - rho_in and (double)P_p, a ray with a non-zero code contributing +0.0, each by the fixed
 *            tree T_{l+1}[r] = T_l[r] + T_l[r ^ (1 << l)], l = 0..5, result T_6[0].  codes uint8[m][64] and edges
 *            float64[m][64][2] = (rho_in, rho_out), 0 for a ray that is not measured: either may be NULL.
 * A ray needs no sample past min(L, k_b + 2 n + 2); the device evaluates none, which changes no result.
 * Host only, usable without a GPU: seunet_airway_wall_rays and _samples return 64; _sweep_points the points one grid sweep takes
 * (one wave per point; tests put more points than that); _directions writes the table, out[2 r] = C_r, out[2 r + 1] = S_r. */
int seunet_airway_wall_rays(void);
int seunet_airway_wall_samples(void);
int seunet_airway_wall_sweep_points(void);
int seunet_airway_wall_directions(double out[128]);
int seunet_airway_walls(const void* ct, int ct_dtype, const int* parsing, int n0, int n1, int n2, double s0, double s1, double s2,
                        double step, double ray_step, int n_search, float min_contrast, int same_label, long long m, const int* table,
                        const double* tangent, unsigned long long* mask, double* sums, unsigned char* codes, double* edges,
                        seunet_stream_t s);

/* ---- surface distances: Hausdorff distance, its percentiles, ASSD and surface Dice in the units of the spacing --
 * The reference computes none of them; the definition is this comment, restated in numpy by tests/surface_oracle.py.
 * a, b: two 0/1 volumes (bytes, non-zero = 1, C-contiguous (n0, n1, n2), extents <= 32767, fewer than 2^31 voxels).
 * border(M) = M and not binary_erosion(M) with the 6-neighbour cross, one iteration, outside the volume = 0 (a set voxel on a face
 * of the volume is a border voxel; MedPy's surface distances with connectivity 1).  d_AB: for every border voxel of A in raster
 * order, sqrt((dt_0^2 + dt_1^2) + dt_2^2) with dt_k = (double)(index_k - coordinate_k) * s_k to the border voxel of B that
 * scipy.ndimage.distance_transform_edt(~border(B), sampling = s) selects, every product and sum rounded on its own: scipy's float64
 * distances bit for bit.  d_BA is the mirror image.  dist = d_AB (n_a values) followed by d_BA (n_b values).  Every result is
 * deterministic and does not depend on the order in which the device executes anything: integer atomics and fixed-shape sums only.
 *
 * seunet_surface_count: packs both masks, forms both borders, counts and scans.  *n_a, *n_b (HOST) receive the numbers of border
 *   voxels and box (6 HOST ints) = {lo0, hi0, lo1, hi1, lo2, hi2}, the bounding box of the non-zero voxels of a or b, high ends
 *   exclusive ({n0, 0, n1, 0, n2, 0} when both are empty).  This call synchronises the stream once, to read those numbers.
 *   workspace: seunet_surface_workspace_bytes(n0, n1, n2), caller-owned, and handed unchanged to seunet_surface_emit.
 * seunet_surface_emit: writes dist (n_a + n_b float64, at most 2^31 - 1) and, unless NULL, voxel (n_a + n_b int32: each border
 *   voxel's linear index in the volume) with the box, n_a and n_b the count call returned; n_a and n_b >= 1 (a mask without voxels
 *   has no surface distances: error).  The distance transforms run inside the box only, which gives the distances of the full
 *   volume bit for bit.  s0, s1, s2: the voxel spacing, positive and finite.  emit_workspace:
 *   seunet_surface_emit_workspace_bytes(hi0 - lo0, hi1 - lo1, hi2 - lo2) (13 bytes per voxel of the box).  Does not synchronise.
 * seunet_surface_summary: out_dev (seunet_surface_summary_bytes(ntol) device bytes, 8-byte aligned) receives, as 64-bit words,
 *   {count_a, count_b, max_a, max_b, sum_a, sum_b, le_a[ntol], le_b[ntol]}: the maxima and sums are float64 (0.0 for an empty
 *   direction), le_x[q] = the number of distances of the direction <= tol[q]; tol: ntol <= 8 HOST doubles.  The sums are formed by
 *   a tree whose shape depends on n_a and n_b alone (the same bits on every run); the bytes behind the record hold its partials.
 * seunet_select_ranks: exact order statistics of float64 device values, FINITE AND NON-NEGATIVE (they are ordered by their 64-bit
 *   patterns).  Request r (nranks <= 8; seg_begin, seg_end, rank: HOST arrays) asks for the element of rank rank[r] (0 = smallest)
 *   among values[seg_begin[r] .. seg_end[r]); segments may overlap; out_dev[r] (device float64) receives it.  A radix select, eight
 *   passes of eight bits for all requests together, without a host round trip between passes; the values are not modified.
 *   n <= 2^31 - 1.  workspace: seunet_select_ranks_workspace_bytes(nranks).
 * None of the last three calls synchronises; all work is ordered on s. */
size_t seunet_surface_workspace_bytes(int n0, int n1, int n2);
int seunet_surface_count(const unsigned char* a, const unsigned char* b, int n0, int n1, int n2, long long* n_a, long long* n_b, int* box,
                         void* workspace, size_t workspace_bytes, seunet_stream_t s);
size_t seunet_surface_emit_workspace_bytes(int b0, int b1, int b2);
int seunet_surface_emit(int n0, int n1, int n2, const int* box, double s0, double s1, double s2, long long n_a, long long n_b,
                        double* dist, int* voxel, const void* count_workspace, size_t count_workspace_bytes, void* emit_workspace,
                        size_t emit_workspace_bytes, seunet_stream_t s);
size_t seunet_surface_summary_bytes(int ntol);
int seunet_surface_summary(const double* dist, long long n_a, long long n_b, const double* tol, int ntol, void* out_dev,
                           seunet_stream_t s);
size_t seunet_select_ranks_workspace_bytes(int nranks);
int seunet_select_ranks(const double* values, long long n, const long long* seg_begin, const long long* seg_end, const long long* rank,
                        int nranks, double* out_dev, void* workspace, size_t workspace_bytes, seunet_stream_t s);

/* ---- component labelling, Euler number, Betti numbers ----------------------------------------------------
 * The reference labels components with skimage.measure.label / scipy.ndimage.label (util.py, tree_parsing.py,
 * atm22_skel_parse.py) and computes no topological number; the definitions are this comment, restated in numpy / scipy by
 * tests/betti_oracle.py.  mask: bytes, non-zero = foreground, C-contiguous (n0, n1, n2), extents >= 1, fewer than 2^31 voxels.
 * connectivity 1, 2, 3 = 6, 18, 26 neighbours (scipy's generate_binary_structure(3, connectivity)).  Integer work only: every
 * result is independent of the order in which the device executes anything.
 *
 * seunet_label: labels (n0 n1 n2 int32) = 0 on the background and 1 .. N on the components, numbered in raster order of each
 *   component's first voxel: scipy.ndimage.label(mask, generate_binary_structure(3, connectivity)) bit for bit.  num_dev (device
 *   int, optional) = N.  workspace: seunet_label_workspace_bytes(n0, n1, n2), caller-owned.  Does not synchronise.
 * seunet_component_table: for the labels and the UNCHANGED workspace of a seunet_label call and its N = num >= 1: size[k] (int64) =
 *   voxels of component k + 1, first[k] (int64) = linear index of its first voxel, box[6 k ..] (int32) = {min0, max0, min1, max1,
 *   min2, max2} of its voxels' coordinates, maxima inclusive.  No cap on N.  Does not synchronise.
 * seunet_remove_small_objects: out (bytes 0 / 1; may alias mask) = the voxels of the components with at least min_size voxels.
 *   workspace: seunet_cc_workspace_bytes(n0, n1, n2).  Does not synchronise.
 *
 * The tile calls take a patch (p0, p1, p2), every extent >= 1 (an extent past the volume's is the volume's): the volume is cut
 * into t0 t1 t2 tiles of that size from the origin, t_k = ceil(n_k / p_k), the last tile of an axis ragged; a tile's numbers are
 * those of the tile cropped out as a volume of its own, and all tiles are done by one fixed set of launches.  The patch
 * (n0, n1, n2) is the whole volume.  connectivity: 3 or 1 (18 neighbours have no dual).
 * seunet_euler: chi_dev (t0 t1 t2 device int64, raster tile order) = the Euler characteristic.  connectivity 3: of the union of
 *   the closed unit cubes of the foreground voxels, V - E + F - C with C the voxels and F, E, V the lattice faces, edges and
 *   vertices that touch at least one of them.  connectivity 1: of the complex whose vertices are the voxels, V' - E' + F' - C' with
 *   the voxels, the face-adjacent pairs, the 2 x 2 squares and the 2 x 2 x 2 cubes that are all foreground.
 *   workspace: seunet_euler_workspace_bytes(n0, n1, n2, p0, p1, p2).
 * seunet_betti: table_dev (t0 t1 t2 x 3 device int32) = (b0, b1, b2) per tile.  b0 = components at `connectivity`; b2 = components
 *   of the complement at the dual connectivity (3 <-> 1) that touch no face of the tile; b1 = b0 + b2 - chi.
 *   workspace: seunet_betti_workspace_bytes(n0, n1, n2, p0, p1, p2).
 * Neither synchronises; all work is ordered on s.  Extent, patch and connectivity errors return before any device work. */
size_t seunet_label_workspace_bytes(int n0, int n1, int n2);
int seunet_label(const unsigned char* mask, int n0, int n1, int n2, int connectivity, int* labels, int* num_dev, void* workspace,
                 size_t workspace_bytes, seunet_stream_t s);
int seunet_component_table(const int* labels, int n0, int n1, int n2, long long num, long long* size, long long* first, int* box,
                           void* workspace, size_t workspace_bytes, seunet_stream_t s);
int seunet_remove_small_objects(const unsigned char* mask, int n0, int n1, int n2, long long min_size, int connectivity,
                                unsigned char* out, void* workspace, size_t workspace_bytes, seunet_stream_t s);
size_t seunet_euler_workspace_bytes(int n0, int n1, int n2, int p0, int p1, int p2);
int seunet_euler(const unsigned char* mask, int n0, int n1, int n2, int p0, int p1, int p2, int connectivity, long long* chi_dev,
                 void* workspace, size_t workspace_bytes, seunet_stream_t s);
size_t seunet_betti_workspace_bytes(int n0, int n1, int n2, int p0, int p1, int p2);
int seunet_betti(const unsigned char* mask, int n0, int n1, int n2, int p0, int p1, int p2, int connectivity, int* table_dev,
                 void* workspace, size_t workspace_bytes, seunet_stream_t s);

/* ---- CT preprocessing: preprocessing.py:26-130 with util.py:95-152 -----------------------------
 * CT volumes are int16, C-contiguous (h, w, z) on the device (the reference's orientation after its transposes), fewer than 2^31
 * voxels; masks are bytes, non-zero = 1.
 * seunet_value_counts: counts[(uint16)(int16)(ct[i] + shift)] += 1 over the n voxels; counts = 65536 device uint32 (zeroed
 *   here).  Bin b holds the value (int16)b.  The 300-bin histograms of preprocessing.py:51 and util.py:99 follow on the host.
 * seunet_shift_clamp: out[i] = (int16)(ct[i] + shift) (numpy's wrapping int16 sum); with clamp != 0, values <= clamp_le
 *   become clamp_to (preprocessing.py:69-71: clamp_le = -800, clamp_to = int16(aaa)).  out may alias ct.
 * seunet_get_l: util.py:120-152 (get_l) for every slice n of range(int(0.05 z) - 1, int(0.95 z)) (n = -1: the last slice):
 *   ct >= T (float64), its largest 8-connected component (ties: first in raster order), that component's 4-connected
 *   holes, relabelled 8-connected, and the largest two of those written as 1 when they have more than min_area pixels (the
 *   reference: 2000).  Every other slice is 0.  workspace: seunet_get_l_workspace_bytes(h, w, z), caller-owned.
 * seunet_mask_combine: out = (a != 0) ^ (b != 0) (op 0) or (a != 0) | (b != 0) (op 1), as 0/1 bytes.
 * seunet_mask_box: box_dev (6 device ints) = {min, max} of the coordinates of the non-zero voxels along axes 0, 1, 2;
 *   {INT_MAX, -1} for an axis of an empty mask.
 * seunet_crop3d: dst = src[box[0]:box[1], box[2]:box[3], box[4]:box[5]] (box: 6 HOST ints, half-open, inside the volume),
 *   elements of elem_bytes = 1 or 2 bytes, dst C-contiguous. */
int seunet_value_counts(const short* ct, long long n, int shift, unsigned int* counts, seunet_stream_t s);
int seunet_shift_clamp(const short* ct, long long n, int shift, int clamp, int clamp_le, int clamp_to, short* out, seunet_stream_t s);
size_t seunet_get_l_workspace_bytes(int h, int w, int z);
int seunet_get_l(const short* ct, int h, int w, int z, double T, int min_area, unsigned char* out, void* workspace,
                 size_t workspace_bytes, seunet_stream_t s);
int seunet_mask_combine(const unsigned char* a, const unsigned char* b, long long n, int op, unsigned char* out, seunet_stream_t s);
int seunet_mask_box(const unsigned char* mask, int h, int w, int z, int* box_dev, seunet_stream_t s);
int seunet_crop3d(const void* src, int elem_bytes, int h, int w, int z, const int* box, void* dst, seunet_stream_t s);

/* ---- whole network: SE_UNet.forward (SE_UNet.py:181-238) and its backward ------------------------------- */
typedef struct seunet_net_desc {
  int batch, in_channel, n_classes;
  int d, h, w;          /* multiples of 8 */
  int width_mult;       /* 1 = reference widths 8/16/32/64 (SE_UNet.py:108-148) */
  int dtype;            /* activation storage: SEUNET_F32 | SEUNET_BF16 | SEUNET_F16 */
  int conv_impl;        /* SEUNET_CONV_MFMA | SEUNET_CONV_NAIVE */
  float negative_slope; /* 0.01 (nn.LeakyReLU default, SE_UNet.py:18) */
  float eps;            /* 1e-5 (nn.InstanceNorm3d default) */
} seunet_net_desc;

int seunet_net_param_count(const seunet_net_desc* desc);
/* name: state_dict key; shape: up to 5 extents (PyTorch layout), ndim 1 or 5 */
int seunet_net_param_info(const seunet_net_desc* desc, int index, char* name, int name_cap, int* shape5, int* ndim);
size_t seunet_net_workspace_bytes(const seunet_net_desc* desc);
/* params: seunet_net_param_count device pointers in registry order.  x: NCDHW f32.  drop1/drop2: DropLayer
 * scale tensors [batch][24] / [batch][12] (NULL = eval mode identity).  pred0/pred1: [batch][n_classes][d][h][w] f32 logits
 * (n_classes 1 .. 8; SE_UNet.py:100,150-151.  Every reference caller uses 1, which keeps the fused head form; more classes run
 * the heads on a general path that materialises the 2-channel side maps, csrc/classes.hip).
 * The workspace keeps everything the backward pass needs; pass the same buffer to seunet_net_backward.
 * pred0 == NULL: inference form (prediction.py:102-103 keeps only the decoder head's output): the encoder head, the side convs of
 * the twelve encoder blocks and their level maps are not evaluated; pred1 is bit-identical; no backward pass may follow. */
int seunet_net_forward(const seunet_net_desc* desc, const float* const* params, const float* x, const float* drop1,
                       const float* drop2, float* pred0, float* pred1, void* workspace, size_t workspace_bytes,
                       seunet_stream_t s);
/* The same forward pass recorded as a HIP graph on exactly these pointers (stream capture on `s`, which must not be the
 * null stream; nothing executes during the capture).  seunet_graph_launch replays it on any stream of the device: the
 * graph reads params / x / drop1 / drop2 and writes pred0 / pred1 / workspace at replay time, so the caller refreshes
 * the CONTENTS of those buffers between replays and keeps the buffers themselves alive and in place.  For the
 * whole-volume inference loop (prediction.py:78-109: the same network call per window, hundreds of times): one graph
 * launch instead of ~150 kernel launches.  Run the eager seunet_net_forward once on the device first (per-kernel
 * one-time attribute setup is not stream work).  seunet_graph_destroy(NULL) is a no-op. */
int seunet_net_forward_capture(const seunet_net_desc* desc, const float* const* params, const float* x, const float* drop1,
                               const float* drop2, float* pred0, float* pred1, void* workspace, size_t workspace_bytes,
                               seunet_stream_t s, void** graph_out);
int seunet_graph_launch(void* graph, seunet_stream_t s);
int seunet_graph_destroy(void* graph);
/* diagnostic: read one intermediate of the last forward that ran on `workspace` back as f32 (which = 0 raw conv output of block
 * `name` [NCDHW], 1 / 2 its InstanceNorm mean / rstd [N][C], 3 the block's output tensor [NCDHW]); *channels = its channel count.
 * `name` may be an x-branch (x33 / x63 / x93; which 0..2): with in_channel <= 2 its raw values exist nowhere and are recomputed
 * from the packed input by the device function the aggregation epilogue uses (params = the forward's parameter list; may be
 * NULL otherwise).  The product path does not call this (tests/flip_census.py and the same-choice gradient gate do). */
int seunet_net_read_tensor(const seunet_net_desc* desc, const float* const* params, const void* workspace, size_t workspace_bytes,
                           const char* name, int which, float* out, int* channels, seunet_stream_t s);
/* Host-only description of the plan's convolutions (no GPU, like seunet_net_workspace_bytes): the index-th convolution block of
 * the network in execution order (the 18 gated 3x3x3 blocks and the 6 aggregation 1x1x1 blocks; dc62 is dead), with the kernel
 * the plan routes each of its passes to.  Returns non-zero past the last convolution (and for a bad descriptor).
 *   dims: the block's level extents, n = batch.  src_c: stored channels of each source tensor; src_is_input: 1 where the source is
 *   the packed network input (it takes no data gradient: a null destination).  cin: logical input channels (in_channel for ec1).
 *   fwd / dgrad / wgrad: SEUNET_KERNEL_* of the forward, data-gradient (meaningful when need_dgrad) and weight-gradient pass.
 *   x_name: the raw-input branch of an aggregation block (x33 / x63 / x93; "" = none), a 1x1x1 conv of the 8-channel packed
 *   input; x_materialised: 1 when it runs as a convolution of its own (in_channel > 2, or the naive path), on x_fwd / x_wgrad;
 *   0 when the aggregation epilogue recomputes it.  src_dist: for a two-source block the byte distance source[1] - source[0]
 *   inside the workspace (what the marching kernels' 32-bit buffer descriptor has to span), 0 otherwise. */
#define SEUNET_KERNEL_NAIVE 0
#define SEUNET_KERNEL_TILED 1     /* implicit GEMM, conv_igemm.hip / wgrad.hip */
#define SEUNET_KERNEL_STREAM 2    /* conv_stream.hip / wgrad_stream.hip */
#define SEUNET_KERNEL_MARCH 3     /* conv_march.hip / wgrad_march.hip */
#define SEUNET_KERNEL_WGRAD1X1 4  /* wgrad_1x1.hip (weight gradient only) */
typedef struct seunet_conv_info {
  char name[16];
  int taps, dilation, level;
  seunet_dims dims;
  int nsrc, src_c[3], src_is_input[3];
  int cin, cout;
  int need_dgrad;
  int fwd, dgrad, wgrad;
  char x_name[16];
  int x_materialised, x_fwd, x_wgrad;
  long long src_dist;
} seunet_conv_info;
int seunet_net_conv_info(const seunet_net_desc* desc, int index, seunet_conv_info* out);
/* grads: device pointers in registry order, each overwritten (NULL = skip).  The dead block dc62
 * (SE_UNet.py:148,230) receives no gradient: its entry is never written. */
int seunet_net_backward(const seunet_net_desc* desc, const float* const* params, const float* g_pred0,
                        const float* g_pred1, const float* drop1, const float* drop2, float* const* grads,
                        void* workspace, size_t workspace_bytes, seunet_stream_t s);
/* the same, recording `decoder_done_event` (a hipEvent_t, or NULL) on the stream once the parameter gradients of the decoder
 * blocks (dc1 .. dc6, dc22, dc42) are final: a data-parallel caller starts reducing that part of the gradient buffer on another
 * stream while the encoder is still being differentiated (the exchange step that replaces DataParallel's reduce, train.py:577). */
int seunet_net_backward_ev(const seunet_net_desc* desc, const float* const* params, const float* g_pred0,
                           const float* g_pred1, const float* drop1, const float* drop2, float* const* grads,
                           void* workspace, size_t workspace_bytes, seunet_stream_t s, void* decoder_done_event);
/* Opt-in gradient with respect to the network input x.  grad_x: NCDHW f32 [batch][in_channel][d][h][w], overwritten (not
 * accumulated).  scratch: a separate caller-owned buffer of seunet_net_input_grad_bytes(desc) bytes, 256-byte aligned, for the
 * per-level f32 x-branch terms (the workspace and seunet_net_workspace_bytes are unchanged).  The parameter gradients are the
 * same bits as seunet_net_backward_ev's; grad_x == NULL IS seunet_net_backward_ev (same launches; scratch unused).
 * dL/dx = convT_ec1(draw_ec1) + W_x33^T d2_x33 + unpool_0(W_x63^T d2_x63 + unpool_1(W_x93^T d2_x93)), max-pool routing to the first
 * maximum of each window of the stored input copy.  In bf16 / fp16 storage it is the gradient with respect to the network's
 * rounded copy of x (the rounding passed straight through).  seunet_net_input_grad_bytes returns 0 and sets
 * seunet_last_error() for a bad descriptor. */
size_t seunet_net_input_grad_bytes(const seunet_net_desc* desc);
int seunet_net_backward_input(const seunet_net_desc* desc, const float* const* params, const float* g_pred0,
                              const float* g_pred1, const float* drop1, const float* drop2, float* const* grads, float* grad_x,
                              void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, seunet_stream_t s,
                              void* decoder_done_event);

/* ---- opt-in timing of the launch groups inside seunet_net_forward/backward (HIP events on the caller's
 * stream; process-wide, meant for one benchmarking thread at a time).  seunet_prof_report writes "tag<TAB>ms<TAB>count" lines and resets; it waits on
 * the recorded events, so call it outside any timed region. */
int seunet_prof_enable(int on);
int seunet_prof_enable_filtered(const char* tag_substring);   /* time only the launch groups whose tag contains it */
int seunet_prof_report(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* SEUNET_HIP_H */
