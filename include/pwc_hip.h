/*
 * pwc_hip.h -- C ABI of libpwc_hip.so, the MI355X (gfx950) replacement for the
 * native half of the reference's PWC-Net inference path.
 *
 * Every entry point
 *   - takes plain device pointers, sizes and an opaque HIP stream handle
 *     (void* == hipStream_t; NULL = the null stream),
 *   - never allocates, frees or synchronises (graph-capturable),
 *   - returns 0 on success, a negative PWC_E* code for an argument the kernel
 *     cannot honour (nothing launched), or a positive hipError_t when the
 *     launch failed.  pwc_last_error() returns a thread-local message.
 *
 * Reference interfaces replaced (paths relative to the reference root):
 *   pwc_corr_fwd        correlation_cuda.forward  models/correlation_package/correlation_cuda.cc:10-87
 *                       (+ channels_first / correlation_forward kernels,
 *                        correlation_cuda_kernel.cu:46-147, launcher :336-427)
 *                       and the fallback semantics of correlation.py:12-40
 *   pwc_corr_bwd        correlation_cuda.backward correlation_cuda.cc:89-167, kernels .cu:150-334
 *   pwc_warp_fwd        PWCDCNet.warp             models/PWCNet.py:141-177
 *   pwc_warp_bwd        autograd of the same (grid_sample backward as used by the training scripts)
 *   pwc_warp_corr81_bwd autograd of corr(c1, warp(c2, s*flo)) + LeakyReLU, PWCNet.py:212-214 etc. (train.py's loss.backward())
 *   pwc_proxy_loss_fwd  ProxyLabelLoss.forward    train_pseudo.py:65-164, train_fundamental.py:62-166 (photometric SSIM + L1
 *                       of the flow-warped image, first-order smoothness)
 *   pwc_proxy_loss_bwd  autograd of the same w.r.t. the flow (train_pseudo's / train_fundamental's loss.backward())
 *   pwc_flow_warp_image_fwd  ProxyLabelLoss.warp  train_pseudo.py:122-157, warp_image train_fundamental.py:80-99
 *   pwc_sup_flow_loss_* MaskedCharbonnier on upsample_flow_to(flow2) train.py:31-48 + :69-72, train2.py:114-122, and
 *                       compute_epe train2.py:100-111 (forward, and backward w.r.t. the low-resolution flow)
 *   pwc_sup_multiscale_loss_*  supervised_multiscale_loss train2.py:124-167 (all levels in one launch, forward and backward)
 *   pwc_epipolar_*      _flow_to_pairs / _ransac_F / build_epipolar_mask_from_flow / epipolar_sampson_loss
 *                       train_fundamental.py:169-382 (the hard epipolar mask and soft Sampson penalty, :459-483)
 *   pwc_fb_metrics      _forward_backward_consistency / _oob_ratio train_pseudo.py:178-236, forward_backward_cycle / oob_ratio
 *                       train_fundamental.py:397-428 (the no-ground-truth validation metrics, on two given flows)
 *   pwc_flow_stats / pwc_flow_color   flow_to_color pwc_extract_flow.py:58-123 (the colour-wheel image save_outputs writes, :182-190)
 *                       and calculate_dominant_direction topview.py:122-134
 *   pwc_flow_compare    compare_flows / print_flow_stats onnx_pth_compare.py:133-201, :225-230 (the parity report of two flow fields)
 *   pwc_flow_quiver     the arrow grid of create_quiver_frame pwc_extract_flow_video.py:94-135 and draw_flow_arrows topview.py:137-178
 *                       (vectors, tips and flags; drawing stays with the caller)
 *   pwc_kitti_augment   KittiFlowDataset.__getitem__ data_processing_or.py:228-294 (reduced augmentation with cv2.warpAffine, random
 *                       crop, horizontal flip) from the raw uint8 frames and the ground truth, only the cropped window computed
 *   pwc_kitti_augment_full   KittiAugmentationPipeline data_processing.py:136-279 (train2.py's collate_fn: crop, flip, rotation,
 *                       translation, brightness / contrast, Gaussian blur) from the same raw inputs
 *   pwc_optim_*         the optimizer step of the four scripts: optim.Adam train.py:129 (under GradScaler.step), train_pseudo.py:423,
 *                       train_fundamental.py:599 (L2 weight decay); clip_grad_norm_ + optim.AdamW train2.py:193, :370
 *   pwc_conv2d_fwd      conv()/predict_flow()     models/PWCNet.py:26-33 (nn.Conv2d 3x3 + LeakyReLU(0.1))
 *   pwc_deconv4x4s2_fwd deconv()                  models/PWCNet.py:35-36 (nn.ConvTranspose2d k4 s2 p1)
 *
 * All tensors are NCHW with contiguous C,H,W planes; only the batch stride is
 * free (in ELEMENTS), so an operand may be a channel slice of a wider
 * [B, Ctot, H, W] arena (this is how the DenseNet concatenations of
 * PWCNet.py:202-264 are done without copies).
 */
#ifndef PWC_HIP_H_
#define PWC_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PWC_ABI_VERSION 13

/* element types */
#define PWC_F32 0
#define PWC_F16 1

/* error codes (negative = argument error, positive = hipError_t) */
#define PWC_OK 0
#define PWC_EINVAL (-1)     /* bad shape / size / null pointer            */
#define PWC_EUNSUPPORTED (-2) /* valid request this build has no kernel for */
#define PWC_EALIGN (-3)     /* pointer or stride alignment not met        */

/* pwc_corr_fwd / pwc_conv2d_fwd flags */
#define PWC_CORR_NORMALIZE 1u /* divide by kernel_size^2*C (correlation_cuda_kernel.cu:104,143) instead of
                                 multiplying by corr_multiply (correlation.py:35-36)              */
#define PWC_ACT_LEAKY 2u      /* fuse LeakyReLU(slope) into the epilogue (PWCNet.py:72,199)          */
#define PWC_CONV_RESIDUAL 4u  /* y += residual (flow2 + dc_conv7(...), PWCNet.py:268)                */
/* pwc_conv3x3_wino4_fwd only */
#define PWC_CONV_SPLIT2 32u   /* y is [4B][Cout][H/2][W/2] (y_bstride = its image stride): image b is written as its four pixel lattices
                                 4b + 2 (oy & 1) + (ox & 1), so that the next, twice-as-dilated layer of the context network runs as
                                 a dilation-1 convolution on 4B small images; pwc_lattice_unsplit_f32 brings a tensor back */
/* pwc_conv2d_f16_fwd only */
#define PWC_CONV_OUT_F32 8u   /* y is float [B][ceil(Cout/8)][Ho][Wo][8] instead of half (flow heads: the values that
                                 carry the flow from level to level stay in fp32)                    */
#define PWC_CONV_SPLIT_W 16u  /* wp comes from pwc_conv3x3_f16_pack_split: hi + lo filters (~22 bits).  Free for Cout <= 16 (the
                                 2-channel heads: the residuals ride in the idle half of the 32-row cout tile); twice the
                                 MFMA passes otherwise (the strict half-precision mode's level-2 / context layers)        */

int pwc_abi_version(void);
/* 0 for the product.  Bits: a kernel source was built with a timing-experiment switch (1 F(4x4) conv, 2 correlation, 4 pipelined
 * correlation, 8 streaming heads): such a library skips work and its results are invalid; never ship or benchmark one. */
int pwc_experiment_mask(void);
const char *pwc_last_error(void);
/* Run-time switches of the kernel selection (process-wide; tests and A/B benchmarks flip them instead of relying on an
 * environment variable being read before first use).  Each option's default comes from the environment variable in brackets:
 *   "conv_wino4" [PWC_CONV_WINO4] 1, "w4_tailsplit" [PWC_W4_TAILSPLIT] 1, "w4_smallsplit" [PWC_W4_SMALLSPLIT] 1,
 *   "w4_small_min_wgs" [PWC_W4_SMALL_MIN_WGS] 160 (workgroups -- tiles x cout groups x Cin slices -- a launch smaller than the chip must reach for
 *   pwc_conv3x3_wino4_preferred to take it; 96 / 64 measured within +-0.6 % / slower on the whole forward),
 *   "corr_pipe" [PWC_CORR_PIPE] 0 (plain correlation on the round-4 pipelined kernels), "corr_roll" [PWC_CORR_ROLL] 1 (their rolling form),
 *   "corr_pipe_min_tiles" [PWC_CORR_PIPE_MIN_TILES] 1024 (8x32 tiles a launch needs for the round-4 kernels),
 *   "corr_small_tiles" [PWC_CORR_SMALL_TILES] 48 (launches of at most this many 8x32 tiles use the small-map correlation kernel, and
 *   pwc_warp_corr81_preferred sends them to pwc_warp_fwd + pwc_corr_fwd; 0: the tiled kernels always),
 *   "head10" [PWC_HEAD10] 1 (fp32 plans: levels too small for pwc_head_upfeat_fwd run predict_flowL + upfeatL as one 10-channel
 *   convolution followed by pwc_upsample_entry_f32; 0: pwc_conv2d_fwd + two pwc_deconv4x4s2_fwd),
 *   "f16_level_corr" [PWC_F16_LEVEL_CORR] 0 (1: the half-precision plans enter a level through pwc_level_corr81_c8_f16 instead of the two
 *   calls it fuses -- same bits, measured slower at batch 16),
 *   "warpcorr_window" [PWC_WARPCORR_WINDOW] 2 (fused warp+correlation on the LDS-window kernel: 2 = C in (28,32] and (60,64], 1 = C <= 32 only, 0 = off),
 *   "stream_slice_wgs" [PWC_STREAM_SLICE_WGS] 512 (pwc_conv2d_fwd, 2-channel flow head on a map of 8..63 8-row x 128-column tiles --
 *   predict_flow2 of one or two pairs, PWCNet.py:263 -- and pwc_head_upfeat_ws_fwd on fewer than 256 tiles: the streaming kernel runs
 *   on Cin slices, as many as bring the launch to this many workgroups, partial sums in the caller's workspace
 *   (pwc_conv2d_workspace_bytes / pwc_head_upfeat_workspace_bytes), fixed-order reduction; 0: one pass / the split-K MFMA kernel),
 *   "head_sliced_min_tiles" [PWC_HEAD_SLICED_MIN_TILES] 14 (fp32 plans: levels of at least this many 8-row x 128-column tiles run predict_flowL +
 *   upfeatL through pwc_head_upfeat_ws_fwd -- on Cin slices below the 64 tiles its one-pass form needs -- instead of the 10-channel
 *   convolution of "head10"; 64: only where the one-pass kernel runs),
 *   "c1_in_arena" [PWC_C1_IN_ARENA] 1 (fp32 plans: the level features of both images live at the arena's batch stride, so that the pyramid's
 *   last convolution writes the first image's straight into their arena slot; 0: dense pyramid buffers and one copy per level),
 *   "w4_stacked" [PWC_W4_STACKED] 1 (pwc_conv3x3_wino4_preferred takes maps shorter than an F(4x4) workgroup where a stacked form -- several
 *   images per workgroup, each with its own border -- serves them: 14x32 for a 32-cout launch, 7x16 for a 64-cout one; the fp32 plan then
 *   runs dc_conv4 / dc_conv5 on the level-4 lattices; 0: refused, the round-4 context path),
 *   "pyr1_wino" [PWC_PYR1_WINO] 1 (fp32 plans: the 16 -> 16 layers conv1aa / conv1b on pwc_pyr1_wino_fwd; 2: both as one
 *   pwc_pyr1_wino_pair_fwd launch -- measured slower, for A/B runs; 0: pwc_conv2d_fwd), "pyr1_wino_min_tiles"
 *   [PWC_PYR1_WINO_MIN_TILES] 512 (8 x 64 tiles a launch needs for it: see pwc_pyr1_wino_preferred) and
 *   "w4_stagger" [PWC_W4_STAGGER] 1 (pwc_conv3x3_wino4_fwd: waves 4-7 of a workgroup place their patch reads and transforms behind other
 *   MFMAs than waves 0-3, their partners on the SIMD -- the same bits; 1: in the forms and launch lengths where it measured faster,
 *   2: in every launch, 0: one schedule for all waves).
 * Unknown name: PWC_EINVAL.  A captured HIP graph keeps the kernels chosen at capture time. */
int pwc_set_option(const char *name, int value);
int pwc_get_option(const char *name, int *value);
/* Name and template arguments of the convolution kernel this thread launched last -- what the tile cost
 * model picked for that layer: "conv3x3_mfma_kernel<MT, NT, stride, dilation, two-per-CU, 0 | 16 = folded tile>" (fp32) or
 * "conv3x3_f16_kernel<MT, NT, stride, dilation, ring, 0>" (fp16).  Every fp32 3x3 path leaves its name: the split-K form
 * ("conv3x3_mfma_splitk_kernel<1, 1, stride, dilation, 0, fold>"), the 16-cout kernel ("conv3x3_mfma16_kernel<NT, CK, ...>"), the
 * 2-channel heads ("stream3x3_kernel<mode, TH, KS, sliced, ...>", "conv3x3_head_kernel<2, ...>"), the Winograd kernels.
 * For benchmarks, profiles and the launch audits. */
const char *pwc_last_conv_kernel(void);

/* Cost volume.  in1,in2: [B,C,H,W]; out: [B,(2*(max_disp/stride2)+1)^2,outH,outW] with
 * outH = ceil((H + 2*pad - 2*((k-1)/2 + max_disp)) / stride1)   (correlation_cuda.cc:25-38).
 * out[b,(tj+r)*D+(ti+r),y,x] = sum_{k x k} sum_c in1p[..]*in2p[..], displacement order tj(dy) outer,
 * ti(dx) inner (correlation_cuda_kernel.cu:107-141; identical to correlation.py:28-29). */
int pwc_corr_fwd(const void *in1, const void *in2, void *out,
                 int B, int C, int H, int W,
                 int pad_size, int kernel_size, int max_disp, int stride1, int stride2,
                 float corr_multiply, int dtype, unsigned flags, float leaky_slope,
                 int64_t in1_bstride, int64_t in2_bstride, int64_t out_bstride,
                 void *stream);

/* warp + cost volume in one kernel for the decoder levels below the coarsest (PWCNet.py:212-213, 226-227, 240-241, 256-257:
 * corr = self.corr(c1, self.warp(c2, up_flow * s)); the warped tensor has no other consumer):
 *   out[b, (dy+4)*9 + (dx+4), y, x] = scale * sum_c in1[b,c,y,x] * warp(x2, flow_scale * flo)[b,c,y+dy,x+dx]   (+ LeakyReLU)
 * with pwc_warp_fwd's sampling / mask rule and pwc_corr_fwd's PWC configuration (pad 4, kernel 1, max displacement 4, strides 1);
 * bit-identical to pwc_warp_fwd followed by pwc_corr_fwd on its tiled kernels (launches of more than "corr_small_tiles" 8x32 tiles;
 * below that pwc_corr_fwd runs its small-map kernel, which sums the channels in another order).  f32 only.  Returns PWC_EUNSUPPORTED (nothing launched) unless
 * W % 4 == 0 and in1 / x2 / out are 16-byte aligned: call the two separate entry points then. */
int pwc_warp_corr81_fwd(const void *in1, const void *x2, const void *flo, void *out, int B, int C, int H, int W,
                        float flow_scale, int align_corners, float mask_threshold,
                        float corr_multiply, unsigned flags, float leaky_slope,
                        int64_t in1_bstride, int64_t x2_bstride, int64_t flo_bstride, int64_t out_bstride, void *stream);
/* 1 when the fused kernel is the faster way to warp + correlate this geometry, 0 for maps of a few tiles (levels 6-4, one-pair
 * inference), where pwc_warp_fwd + pwc_corr_fwd (small-map kernel) win by ~3x, the extra launch included. */
int pwc_warp_corr81_preferred(int B, int C, int H, int W);

/* Gradients of pwc_corr_fwd w.r.t. in1 and in2 (no fused activation; same scale rule as forward), for ANY
 * (pad_size, kernel_size, max_disp, stride1, stride2) like the reference's backward (correlation_cuda_kernel.cu:150-334);
 * grad_out: [B, D*D, outH, outW] contiguous, in*, grad_in*: [B,C,H,W] contiguous.  Gather form with a fixed summation
 * order (deterministic, no atomics).  PWC-Net's configuration in fp32 runs an LDS-tiled kernel (one thread per pixel,
 * 81 + 81 grad_out values in registers, both inputs streamed through LDS with their halos). */
int pwc_corr_bwd(const void *in1, const void *in2, const void *grad_out, void *grad_in1, void *grad_in2,
                 int B, int C, int H, int W,
                 int pad_size, int kernel_size, int max_disp, int stride1, int stride2,
                 float corr_multiply, int dtype, unsigned flags,
                 void *stream);

/* Gradients of pwc_warp_corr81_fwd (flo != NULL) or of pwc_corr_fwd in PWC-Net's configuration (flo == NULL: level 6, no warp),
 * the fused LeakyReLU included, in one pass (csrc/pwc_warp_corr_bwd.hip):
 *   y = act(scale * sum_c c1[p,c] * warp(c2, flow_scale * flo)[p+d,c])    (pad 4, max displacement 4, strides 1, 81 displacements)
 * c1, c2: [B,C,H,W]; flo: [B,2,H,W] or NULL; y, gy: [B,81,H,W] (y = the forward's ACTIVATED output, read for the LeakyReLU mask
 * y > 0; only with PWC_ACT_LEAKY, may be NULL otherwise); flags, corr_multiply, leaky_slope, flow_scale, align_corners and
 * mask_threshold as in the forward.  Outputs dense (contiguous): grad_c1, grad_c2 [B,C,H,W], grad_flo [B,2,H,W] (unused with
 * flo == NULL).  Input batch strides in elements, C/H/W planes dense.  Semantics of autograd on the reference's expression: the
 * warp's validity mask is a constant (PWCNet.py:174-175 thresholds it in place), d/dflo goes through the sample coordinates.
 * Bit-reproducible: grad_c1 and the warped tensor's gradient are gathers with a fixed order; the scatter into grad_c2 (warp form)
 * accumulates 64-bit fixed-point integers in `workspace` (>= pwc_warp_corr81_bwd_workspace_bytes, 8-byte aligned; required with
 * flo, unused without), scale 2^(39 - floor(log2 M)) with M = 81 * max|gy| * |scale| * max(1,|slope|) * max|c1|, a bound on every
 * contribution (resolution 2^-39 of M; 2^23 contributions of the bound per element before an int64 could wrap).  Non-finite gy or
 * c1: float atomics for that call's grad_c2 (no synchronisation; last bits then order-dependent), as pwc_warp_bwd.
 * The workspace also holds the per-16-channel-chunk partial sums of grad_flo, added in chunk order by a final pass.
 * f32 only.  PWC_EUNSUPPORTED (nothing launched) unless every operand is 4-byte aligned, max(C,81)*H*W < 2^31 and the grid fits. */
int64_t pwc_warp_corr81_bwd_workspace_bytes(int B, int C, int H, int W);
int pwc_warp_corr81_bwd(const void *c1, const void *c2, const void *flo, const void *y, const void *gy,
                        void *grad_c1, void *grad_c2, void *grad_flo, int B, int C, int H, int W,
                        float flow_scale, int align_corners, float mask_threshold, float corr_multiply,
                        unsigned flags, float leaky_slope,
                        int64_t c1_bstride, int64_t c2_bstride, int64_t flo_bstride, int64_t y_bstride, int64_t gy_bstride,
                        void *workspace, int64_t workspace_bytes, void *stream);

/* Self-supervised proxy-label loss (ABI v13 additions, csrc/pwc_proxy_loss.hip), restating train_pseudo.py:65-164 (ssim_eps 0) and
 * train_fundamental.py:62-166 (ssim_eps 1e-12, optional valid_mask):
 *   up     = interpolate(flow, (H,W), bilinear, align_corners=True) * (W/w, H/h)   (flow itself when (h,w) == (H,W));
 *   y_c    = grid_sample(img2, x + up, bilinear, border, align_corners=True)         (train_pseudo.py:122-157, :80-99);
 *   map    = 0.85 mean_c clamp((1 - SSIM_c(img1, y)) / 2, 0, 1) + 0.15 mean_c |img1 - y|, SSIM on avg_pool2d(3, 1, 1)
 *            (zero padding, divisor 9) moments with C1 = 0.01^2, C2 = 0.03^2 and + ssim_eps in the denominator (:87-101, :139-150);
 *   photo  = mean(map), or with a mask sum(map * [m > 0.5]) / max(sum [m > 0.5], 1) (:117-126);
 *   smooth = mean|d/dx flow| + mean|d/dy flow| on the low-resolution flow (:103-107, :152-156);
 *   total  = alpha_photo * photo + alpha_smooth * smooth.
 * flow [B,2,h,w], img1 / img2 [B,C,H,W] f32 (dense C,H,W planes, batch strides in elements); mask [B,H,W] (plane dense, batch
 * stride mask_bstride) stored as f32 (mask_u8 = 0) or u8 (mask_u8 = 1), or NULL.  The sample point is computed in fp32 as
 *   rh = (float)(h-1) / (float)(H-1);  fy = rh * (float)Y;  y0 = (int)fy;  y1 = y0 + (y0 < h-1);  ly1 = fy - (float)y0;  ly0 = 1 - ly1
 *   (x alike);  up_x = (ly0 * (lx0 * f00 + lx1 * f01) + ly1 * (lx0 * f10 + lx1 * f11)) * (float)((double)W / w)  (v alike with H / h);
 *   px = (float)X + up_x;  ix = min(max(px, 0), W-1);  x0 = floor(ix);  tx = ix - x0   (y alike)
 * with no fused multiply-add (the library is built with -ffp-contract=off); the reference's linspace + normalise + unnormalise
 * chain computes the same point in exact arithmetic.
 * pwc_proxy_loss_fwd writes float out[3] = {total, photo, smooth} in device memory; partial sums per 16 x 64 tile in fp64, added in
 * a fixed order.  pwc_proxy_loss_bwd reads grad_out[3] = {g_total, g_photo, g_smooth} from device memory (no host sync) and writes
 * grad_flow [B,2,h,w] (dense) = (g_total * alpha_photo + g_photo) d photo / d flow + (g_total * alpha_smooth + g_smooth) d smooth / d flow,
 * the gradient autograd derives from the reference's expression: 0 where a sample coordinate is clipped (<= 0 or >= size-1),
 * clamp passes on its closed interval, |0| has gradient 0; the images and the mask get none.  It recomputes the warp and the
 * moments per tile (nothing is kept from the forward) and gathers grad_flow in a fixed order: both entries are bit-reproducible.
 * workspace: device, 8-byte aligned; the forward needs pwc_proxy_loss_fwd_workspace_bytes (32 bytes per 16 x 64 tile), the backward
 * pwc_proxy_loss_workspace_bytes (grad_up [B,2,H,W] + 256 bytes; also >= the forward's, so one buffer serves both entries).
 * The backward's gather gives one lane per low-resolution pixel about (2H/h) x (2W/w) full-resolution pixels to sum: fine at the
 * scripts' 4x upsampling, slow (correct) at extreme ratios such as a 2 x 2 flow.
 * Null operands (mask excepted) / bad shapes / short strides / short workspace: PWC_EINVAL before any launch.
 * PWC_EUNSUPPORTED (nothing launched) when H, W, h or w < 2, H < h, W < w, an f32 operand is not 4-byte aligned, C*H*W >= 2^31,
 * B > 65535 or H > 16 * 65535. */
int64_t pwc_proxy_loss_workspace_bytes(int B, int C, int H, int W, int h, int w);
int64_t pwc_proxy_loss_fwd_workspace_bytes(int B, int C, int H, int W, int h, int w);
int pwc_proxy_loss_fwd(const void *flow, const void *img1, const void *img2, const void *mask, int mask_u8,
                       void *out, int B, int C, int H, int W, int h, int w,
                       float alpha_photo, float alpha_smooth, float ssim_eps,
                       int64_t flow_bstride, int64_t img1_bstride, int64_t img2_bstride, int64_t mask_bstride,
                       void *workspace, int64_t workspace_bytes, void *stream);
int pwc_proxy_loss_bwd(const void *flow, const void *img1, const void *img2, const void *mask, int mask_u8,
                       const void *grad_out, void *grad_flow, int B, int C, int H, int W, int h, int w,
                       float alpha_photo, float alpha_smooth, float ssim_eps,
                       int64_t flow_bstride, int64_t img1_bstride, int64_t img2_bstride, int64_t mask_bstride,
                       void *workspace, int64_t workspace_bytes, void *stream);
/* warp / warp_image of the same scripts (train_pseudo.py:122-157, train_fundamental.py:80-99), forward only, any C:
 * out [B,C,H,W] = img sampled at the point above (flow [B,2,h,w], upsampled when (h,w) != (H,W)).  Same declines as the loss. */
int pwc_flow_warp_image_fwd(const void *img, const void *flow, void *out, int B, int C, int H, int W, int h, int w,
                            int64_t img_bstride, int64_t flow_bstride, int64_t out_bstride, void *stream);

/* Supervised flow losses (ABI v13 additions, csrc/pwc_sup_loss.hip), restating train.py / train2.py.  fp32, fixed-order fp64
 * partial sums, no float atomics: bit-reproducible.  torch's index arithmetic in fp32 (no fused multiply-add):
 *   bilinear, align_corners=False: scale = (float)in / (float)out;  s = max(scale * ((float)dst + 0.5) - 0.5, 0);  i0 = (int)s;
 *     i1 = i0 + (i0 < in-1);  l1 = s - i0;  l0 = 1 - l1;   nearest: min((int)floorf((float)dst * scale), in-1).
 * pwc_sup_flow_loss_fwd: masked Charbonnier / EPE of pred [B,2,h,w] upsampled to gt [B,2,H,W] (train.py:31-48 + :69-72 with
 *   upsample_flow_to of data_processing_or.py:300-310, train2.py:114-122, compute_epe train2.py:100-111 on :202-213):
 *   up = interpolate(pred, (H,W), bilinear, align_corners=False) * (float)(W/w, H/h)  (2 <= h <= H, 2 <= w <= W; (h,w) == (H,W)
 *   is the plain loss), epe = sqrt(|up - gt|^2 + (float)(eps^2));  mask [B,H,W] (a [B,1,H,W] mask is the same plane) f32
 *   (mask_u8 = 0) or u8 (mask_u8 = 1), or NULL (every pixel, weight 1).  mask_rule 0: loss = sum(epe [m > 0.5]) / max(sum [m > 0.5], 1)
 *   (MaskedCharbonnier); mask_rule 1: loss = sum(epe m) / (sum m + 1e-8) (compute_epe; eps 0); no mask: the mean.  Writes float
 *   out[2] = {loss, den} in device memory; the upsampled flow is sampled on the fly, never written.
 * pwc_sup_flow_loss_bwd: grad_pred [B,2,h,w] (dense) = grad_out[0] d loss / d pred, reading grad_out[0] and den = fwd_out[1] (the
 *   forward's out) from device memory (no host sync); den gets no gradient.  A row pass sums along X into [B,2,H,w] fp64 in the
 *   workspace, a column pass along Y: each low-resolution pixel gathers the full-resolution pixels whose taps use it, in order.
 * pwc_sup_flow_loss_workspace_bytes: the forward's (backward = 0: 16 bytes per 1024 pixels) or the backward's (backward = 1; also
 *   >= the forward's).
 * pwc_sup_multiscale_loss_fwd: supervised_multiscale_loss (train2.py:124-167) over L <= 8 levels, one launch for all of them.
 *   Host arrays: preds[L] device pointers to [B,2,h_l,w_l] f32 (batch strides pred_bstrides[L]; NULL = dense), level_hw[2L] =
 *   (h_l, w_l), weights[L].  gt [B,2,H,W] f32, mask [B,H,W] f32 / u8 or NULL (weight 1), images [B,6,H,W] f32 = (im1, im2) (read
 *   only when a lambda is > 0; may be NULL otherwise).  Per level: gt_s = bilinear downsample of gt * (1 / (float)(W/w), 1 /
 *   (float)(H/h)), mask_s = nearest mask (raw), charb = sum(sqrt(|pred - gt_s|^2 + eps^2) [mask_s > 0.5]) / max(sum [.], 1);
 *   lambda_photo > 0: photo = sum_c |im1_s - grid_sample(im2_s, (x + u, y + v), bilinear, zeros, align_corners=True)| mask_s /
 *   (sum mask_s + 1e-8) (:44-77); lambda_smooth > 0: smooth = mean(|dx pred| exp(-mean_c |dx im1_s|)) + the same along y (:80-97);
 *   im1_s / im2_s are bilinear (align_corners=False) downsamples, written to the workspace by a resize launch.
 *   out float [1 + 3L] in device memory = {total = sum_l w_l lvl_l, lvl_l = charb + lambda_photo photo + lambda_smooth smooth,
 *   den_c[L] = max(sum [mask_s > 0.5], 1), den_p[L] = sum mask_s + 1e-8}.
 * pwc_sup_multiscale_loss_bwd: grads[L] (host array of device pointers, dense [B,2,h_l,w_l]) = grad_out[0] d total / d pred_l,
 *   elementwise, reading grad_out[0] and the forward's out (fwd_out, for den_c / den_p) from device memory; photometric slopes of the
 *   zero-padded im2_s with grid_sample's floor-based taps, sign(0) = 0.  Same arguments and workspace as the forward.
 * pwc_sup_multiscale_loss_workspace_bytes: partial sums (48 bytes per 1024 pixels) + with_images: im1_s / im2_s of every level.
 * Null operands / bad shapes / short strides / short workspace / negative eps or lambda: PWC_EINVAL before any launch.
 * PWC_EUNSUPPORTED (nothing launched) when h or w < 2, h > H, w > W, L > 8, an f32 operand is not 4-byte aligned, 6*H*W >= 2^31
 * (2*H*W for the flow loss) or B > 65535. */
int64_t pwc_sup_flow_loss_workspace_bytes(int B, int H, int W, int h, int w, int backward);
int pwc_sup_flow_loss_fwd(const void *pred, const void *gt, const void *mask, int mask_u8, int mask_rule, void *out,
                          int B, int H, int W, int h, int w, double eps, int64_t pred_bstride, int64_t gt_bstride,
                          int64_t mask_bstride, void *workspace, int64_t workspace_bytes, void *stream);
int pwc_sup_flow_loss_bwd(const void *pred, const void *gt, const void *mask, int mask_u8, int mask_rule,
                          const void *fwd_out, const void *grad_out, void *grad_pred, int B, int H, int W, int h, int w,
                          double eps, int64_t pred_bstride, int64_t gt_bstride, int64_t mask_bstride, void *workspace,
                          int64_t workspace_bytes, void *stream);
int64_t pwc_sup_multiscale_loss_workspace_bytes(int B, int H, int W, int L, const int *level_hw, int with_images);
int pwc_sup_multiscale_loss_fwd(const void *const *preds, const int64_t *pred_bstrides, const int *level_hw,
                                const float *weights, int L, const void *gt, const void *mask, int mask_u8,
                                const void *images, void *out, int B, int H, int W, double eps, float lambda_photo,
                                float lambda_smooth, int64_t gt_bstride, int64_t mask_bstride, int64_t img_bstride,
                                void *workspace, int64_t workspace_bytes, void *stream);
int pwc_sup_multiscale_loss_bwd(const void *const *preds, const int64_t *pred_bstrides, const int *level_hw,
                                const float *weights, int L, const void *gt, const void *mask, int mask_u8,
                                const void *images, const void *fwd_out, const void *grad_out, void *const *grads,
                                int B, int H, int W, double eps, float lambda_photo, float lambda_smooth,
                                int64_t gt_bstride, int64_t mask_bstride, int64_t img_bstride, void *workspace,
                                int64_t workspace_bytes, void *stream);

/* Epipolar hard mask and soft Sampson penalty (ABI v13 additions, csrc/pwc_epipolar.hip), restating train_fundamental.py:169-382
 * as called at :459-483.  All geometry in fp64; integer or fixed-order fp64 reductions, no float atomics: bit-reproducible.
 * flow [B,2,H,W] f32 (dense planes, batch stride in elements).
 * pwc_epipolar_pairs: _flow_to_pairs (:169-194).  pts f64 [B,cap,4] = (x, y, x + fu, y + fv) of the grid points
 *   mgrid[0:H:stride, 0:W:stride] (row-major, cap = ceil(H/stride) * ceil(W/stride)) whose endpoints are finite and whose image
 *   mask (u8 or f32 [B,H,W], != 0; NULL = none) is set, packed in order; npts int32 [B] = N_b.
 * pwc_epipolar_ransac: _ransac_F (:236-258) on those pairs.  idx int32 [iters,8] per sample (batch stride idx_bstride elements,
 *   0 = one table for all) is numpy's rng.choice(N_b, 8, replace=False) sequence, drawn by the caller; hypothesis i fits row i by
 *   _eight_point_F (:211-225; the vector of the 8th-largest singular value of the 8 x 9 system, as numpy's thin SVD returns),
 *   counts[B,iters] int32 = #{d < thresh}; the first strictly largest count wins; F_out f64 [B,9] = the refit on its inliers
 *   (vector of the min(n,9)-th largest singular value), ok_out int32 [B] = 0 when N_b < 8 or the best count < 8 (F_out = 0 then),
 *   best_out int32 [B] (may be NULL) = the winning index (-1 when N_b < 8).  workspace: pwc_epipolar_ransac_workspace_bytes.
 * pwc_epipolar_distance: dist f64 [B,H,W] = Sampson d of every pixel (:285-296; x / (x_2 + 1e-12) included) for F f64 [.,9]
 *   (F_bstride 9 per sample, 0 = one F).
 * pwc_epipolar_mask: build_epipolar_mask_from_flow (:261-327) from F f64 [B,9] and ok int32 [B]: thr = min(tau, np.quantile(d_finite,
 *   keep_ratio)) (linear method, numpy's _lerp), mask = finite & d <= thr, relaxed to min(tau, quantile(min_keep)) when
 *   mean(mask) < min_keep (each step only when its ratio is in (0,1)); mask_out u8 [B,H,W]; thr_out f64 [B] (NaN where the mask is
 *   all true: fit failed or no finite d); dist_out (may be NULL) receives d.  workspace: pwc_epipolar_mask_workspace_bytes.
 * pwc_epipolar_loss_fwd / _bwd: epipolar_sampson_loss (:331-382) with F f64 [.,9] rounded to f32 (F_bstride 9 or 0), ok int32
 *   (NULL = all; ok_bstride 1 or 0: samples with ok == 0 select nothing), mask u8 / f32 [B,H,W] (> 0.5; NULL = all pixels);
 *   robust 0 = huber(delta), 1 = l1, 2 = plain mean; out f32 [1] = weight * mean over the selected pixels (0 when none).  The
 *   backward reads grad_out f32 [1] from device memory and writes grad_flow [B,2,H,W] (dense; 0 off the selection).  Both use
 *   pwc_epipolar_loss_workspace_bytes.
 * Null operands / bad shapes / short strides / short workspace: PWC_EINVAL before any launch.  PWC_EUNSUPPORTED (nothing launched)
 * for misaligned operands (f32 / int32 4-byte, f64 8-byte), 2*H*W >= 2^31, B > 65535, NaN thresholds or delta <= 0. */
int pwc_epipolar_pairs(const void *flow, const void *mask, int mask_u8, void *pts, void *npts, int B, int H, int W, int stride,
                       int64_t flow_bstride, int64_t mask_bstride, void *stream);
int64_t pwc_epipolar_ransac_workspace_bytes(int B, int iters);
int pwc_epipolar_ransac(const void *pts, const void *npts, int cap, const void *idx, int64_t idx_bstride, int B, int iters,
                        double thresh, void *F_out, void *ok_out, void *best_out, void *counts, void *workspace,
                        int64_t workspace_bytes, void *stream);
int pwc_epipolar_distance(const void *flow, const void *F, int64_t F_bstride, void *dist, int B, int H, int W,
                          int64_t flow_bstride, void *stream);
int64_t pwc_epipolar_mask_workspace_bytes(int B, int H, int W);
int pwc_epipolar_mask(const void *flow, const void *F, const void *ok, void *mask_out, void *thr_out, void *dist_out,
                      int B, int H, int W, double tau, double keep_ratio, double min_keep, int64_t flow_bstride,
                      void *workspace, int64_t workspace_bytes, void *stream);
int64_t pwc_epipolar_loss_workspace_bytes(int B, int H, int W);
int pwc_epipolar_loss_fwd(const void *flow, const void *F, int64_t F_bstride, const void *ok, int64_t ok_bstride,
                          const void *mask, int mask_u8, void *out, int B, int H, int W, int robust, double delta, double weight,
                          int64_t flow_bstride, int64_t mask_bstride, void *workspace, int64_t workspace_bytes, void *stream);
int pwc_epipolar_loss_bwd(const void *flow, const void *F, int64_t F_bstride, const void *ok, int64_t ok_bstride,
                          const void *mask, int mask_u8, const void *grad_out, void *grad_flow, int B, int H, int W, int robust,
                          double delta, double weight, int64_t flow_bstride, int64_t mask_bstride, void *workspace,
                          int64_t workspace_bytes, void *stream);

/* No-ground-truth validation metrics (ABI v13 additions, csrc/pwc_fb_metrics.hip): forward-backward cycle consistency
 * (_forward_backward_consistency train_pseudo.py:178-193, forward_backward_cycle train_fundamental.py:397-409) and the
 * out-of-bounds ratio (_oob_ratio train_pseudo.py:210-236, oob_ratio train_fundamental.py:412-428) in one pass, nothing
 * image-sized written.  flow12 / flow21 [B,2,h,w] f32 (dense planes, batch strides in elements); flow21 may be NULL.
 * Per pixel (b, Y, X) of the H x W grid, in fp32 with no fused multiply-add (the arithmetic of pwc_proxy_loss_fwd above):
 *   1. a = up(flow12)(Y, X):  up(f)(Y, X) = f[Y, X] when (h,w) == (H,W), otherwise
 *        rh = (float)(h-1) / (float)(H-1);  fy = rh * (float)Y;  y0 = (int)fy;  y1 = y0 + (y0 < h-1);  ly1 = fy - (float)y0;
 *        ly0 = 1 - ly1  (x alike);  u = ly0 * (lx0 * f00 + lx1 * f01) + ly1 * (lx0 * f10 + lx1 * f11);
 *        up.x = u * (float)((double)W / w)  (up.y alike with (float)((double)H / h))           -- upsample_flow_to of both scripts;
 *   2. px = (float)X + a.x;  py = (float)Y + a.y;  the pixel is OUT OF BOUNDS when px < 0 || px > W-1 || py < 0 || py > H-1
 *        (the pixel form of the scripts' x < -1 | x > 1 | y < -1 | y > 1 on the normalised grid);
 *   3. ix = min(max(px, 0), W-1);  x0 = floor(ix);  tx = ix - x0;  x1 = min(x0 + 1, W-1)  (y alike);  the four taps are
 *        v00 = up(flow21)(y0, x0), v01 = up(flow21)(y0, x1), v10 = up(flow21)(y1, x0), v11 = up(flow21)(y1, x1), each evaluated
 *        from the [h,w] field as in step 1;  wv = (1-ty) * ((1-tx) * v00 + tx * v01) + ty * ((1-tx) * v10 + tx * v11)
 *        per component -- grid_sample(bilinear, border, align_corners=True) of the scripts' warp / warp_image;
 *   4. cycle += |a.x + wv.x| + |a.y + wv.y|   (the sum of the two fp32 magnitudes is added in fp64).
 * out2 (device, float[2]) = {cycle / (B*2*H*W), oob_count / (B*H*W)}; with flow21 == NULL only the count is taken (the scripts'
 * stand-alone oob_ratio) and out2[0] = 0.  Each 16 x 64 tile leaves {fp64 cycle sum, int64 count} in the workspace, summed in a
 * fixed tree order, and one final workgroup adds the tiles in order: no atomics, bit-reproducible, no host synchronisation.
 * workspace: device, 8-byte aligned, pwc_fb_metrics_workspace_bytes(B, H, W) = 16 + 16 bytes per tile (-1 for a non-positive
 * size).  After the launch its first 16 bytes hold the raw totals: the fp64 cycle sum, then the int64 out-of-bounds count.
 * PWC_EINVAL, nothing launched: null flow12 / workspace / out2, non-positive sizes, H, W, h or w < 2, H < h, W < w,
 * B*2*H*W >= 2^31, B > 65535, H > 16 * 65535, a batch stride below 2*h*w, an operand not 4-byte aligned, a workspace that is too
 * small or not 8-byte aligned. */
int64_t pwc_fb_metrics_workspace_bytes(int B, int H, int W);
int pwc_fb_metrics(const void *flow12, const void *flow21, int B, int h, int w, int H, int W,
                   int64_t flow12_bstride, int64_t flow21_bstride,
                   void *workspace, int64_t workspace_bytes, void *out2, void *stream);

/* Backward warp of x by (flow_scale * flo): bilinear, zero padding, times the validity mask
 * [sum of in-bounds bilinear weights >= mask_threshold]  (PWCNet.py:141-177).
 * x,out: [B,C,H,W]; flo: [B,2,H,W] (u then v).  align_corners=0 reproduces the reference as executed
 * by torch>=1.3: x_src = (x+u)*W/(W-1) - 0.5. */
int pwc_warp_fwd(const void *x, const void *flo, void *out,
                 int B, int C, int H, int W,
                 float flow_scale, int align_corners, float mask_threshold, int dtype,
                 int64_t x_bstride, int64_t flo_bstride, int64_t out_bstride,
                 void *stream);

/* Gradients of pwc_warp_fwd w.r.t. x and flo (contiguous f32 tensors).  The validity mask is a constant, as in the
 * reference, whose in-place thresholding (PWCNet.py:174-175) cuts the mask's graph; what autograd derives for
 * PWCNet.py:141-177 is otherwise reproduced: d/dx through the bilinear taps (a scatter: which output pixels sample a source
 * pixel depends on the flow), d/dflo through the sample coordinates.
 * workspace (device, 8-byte aligned, >= pwc_warp_bwd_workspace_bytes): the scatter accumulates 64-bit FIXED-POINT integers
 * there (integer addition is associative -> bit-reproducible grad_x whatever order the atomics arrive in; resolution 2^-40
 * of the largest |grad_out|) and grad_x is written once at the end.  workspace == NULL: grad_x is zeroed and accumulated
 * with float atomics like torch's grid_sample backward (summation order, hence the last bits, not fixed).
 * Limits of the fixed-point form: (1) one contribution is at most 2^41 in magnitude, so a source pixel that collects more
 * than 2^22 (4 194 304) contributions of the largest |grad_out| would wrap its int64 -- more output pixels than that sampling
 * ONE source pixel; (2) a non-finite grad_out (Inf / NaN) has no fixed-point form: the call then falls back, on the device and
 * without synchronising, to the float-atomic accumulation for the whole tensor, so Inf / NaN reach grad_x exactly as in the
 * float path (that call is not bit-reproducible). */
int64_t pwc_warp_bwd_workspace_bytes(int B, int C, int H, int W);
int pwc_warp_bwd(const void *x, const void *flo, const void *grad_out, void *grad_x, void *grad_flo,
                 int B, int C, int H, int W,
                 float flow_scale, int align_corners, float mask_threshold, int dtype,
                 void *workspace, int64_t workspace_bytes, void *stream);

/* Bytes needed for the packed (kernel-native) form of a [Cout,Cin,3,3] filter bank. */
int64_t pwc_conv3x3_packed_bytes(int Cin, int Cout, int dtype);
/* Repack w:[Cout,Cin,3,3] (device, NCHW filter layout of nn.Conv2d) into wp (device). */
int pwc_conv3x3_pack(const void *w, void *wp, int Cin, int Cout, int dtype, void *stream);

/* 3x3 convolution, padding == dilation (so H,W are preserved at stride 1; Hout = (H-1)/stride+1),
 * + bias, optional LeakyReLU and residual.  x:[B,Cin,H,W], y:[B,Cout,Hout,Wout],
 * wp = output of pwc_conv3x3_pack, bias:[Cout] f32, residual: same geometry as y or NULL.
 * workspace (device, 4-byte aligned, may be NULL): scratch for the split-K route taken by layers with few
 * output tiles and many input channels (pyramid levels 6-4, batch-1 inference): partial sums per Cin range,
 * then a fixed-order reduction (deterministic).  A layer whose pwc_conv2d_workspace_bytes() exceeds
 * workspace_bytes runs unsplit -- same result up to fp32 summation order.  One workspace may be shared by all
 * layers launched on the same stream. */
int pwc_conv2d_fwd(const void *x, const void *wp, const void *bias, const void *residual, void *y,
                   int B, int Cin, int H, int W, int Cout,
                   int stride, int dilation, int dtype, unsigned flags, float leaky_slope,
                   int64_t x_bstride, int64_t y_bstride, int64_t res_bstride,
                   void *workspace, int64_t workspace_bytes,
                   void *stream);
/* Bytes of workspace the split-K route of this layer needs (0: the layer never splits; <0: bad shape). */
int64_t pwc_conv2d_workspace_bytes(int B, int Cin, int H, int W, int Cout, int stride, int dilation);

/* ---- Winograd F(2x2,3x3) route of the same operator (nn.Conv2d 3x3, stride 1, padding = dilation + LeakyReLU,
 * PWCNet.py:26-33), fp32 in / fp32 MFMA accumulation / fp32 out: 16 multiplications per 2x2 outputs instead of 36.
 * The result differs from pwc_conv2d_fwd only by fp32 rounding (the transforms add and halve; tests bound it).
 * up = pwc_conv3x3_wino_pack(w) holds G g Gt per (cout, cin) in the kernel's LDS order [chunk of 4 cin][16][2][CoutP][2].
 * A dilated layer runs as dilation^2 ordinary convolutions on the pixel lattices (y mod D, x mod D).
 * x:[B,Cin,H,W], y:[B,Cout,H,W] with free batch strides (elements); flags: PWC_ACT_LEAKY only. */
int64_t pwc_conv3x3_wino_packed_bytes(int Cin, int Cout);
/* 1 when this route is expected to beat pwc_conv2d_fwd for the layer (enough workgroups for 256 CUs, Cout >= 32), else 0 */
int pwc_conv3x3_wino_preferred(int B, int Cin, int H, int W, int Cout, int dilation);
int pwc_conv3x3_wino_pack(const void *w, void *up, int Cin, int Cout, void *stream);
int pwc_conv3x3_wino_fwd(const void *x, const void *up, const void *bias, void *y,
                         int B, int Cin, int H, int W, int Cout, int dilation, unsigned flags, float leaky_slope,
                         int64_t x_bstride, int64_t y_bstride, void *workspace, int64_t workspace_bytes, void *stream);
/* workspace (device, may be NULL): scratch for the split-K form taken by launches that would leave most CUs idle (levels 5-4);
 * pwc_conv3x3_wino_workspace_bytes() bytes, shareable with pwc_conv2d_fwd's workspace on one stream; without it the layer runs unsplit */
int64_t pwc_conv3x3_wino_workspace_bytes(int B, int Cin, int H, int W, int Cout, int dilation);

/* The same operator by Winograd F(4x4,3x3) (csrc/pwc_conv_wino4.hip, round 3): 36 multiplications per 4x4 outputs -- 1.78x fewer
 * MFMA passes than F(2x2,3x3) -- at ~6x (rms) the fp32 rounding error of F(2x2) (4e-5 instead of 2e-6 at the largest on unit-scale
 * data with 565 input channels).  Dilation 1, W % 4 == 0, 16-byte aligned x / y with batch strides that are multiples of 4
 * (PWC_EUNSUPPORTED / PWC_EALIGN otherwise).  up = pwc_conv3x3_wino4_pack(w): G g Gt (6x6 per filter, computed in double) in the
 * kernel's LDS order [chunk of 4 cin][9 groups of 4 positions][cin][CoutP][4], pwc_conv3x3_wino4_packed_bytes() bytes (4x the filter).
 * pwc_conv3x3_wino4_preferred: the measured rule for when this route beats pwc_conv3x3_wino_fwd (large, well-filled maps).
 * flags: PWC_ACT_LEAKY. */
int64_t pwc_conv3x3_wino4_packed_bytes(int Cin, int Cout);
int pwc_conv3x3_wino4_preferred(int B, int Cin, int H, int W, int Cout, int dilation);
int pwc_conv3x3_wino4_pack(const void *w, void *up, int Cin, int Cout, void *stream);
int pwc_conv3x3_wino4_fwd(const void *x, const void *up, const void *bias, void *y,
                          int B, int Cin, int H, int W, int Cout, int dilation, unsigned flags, float leaky_slope,
                          int64_t x_bstride, int64_t y_bstride, void *workspace, int64_t workspace_bytes, void *stream);
/* workspace (device, 16-byte aligned, may be NULL): pwc_conv3x3_wino4_workspace_bytes() bytes, shareable with the other convolutions'
 * workspaces on one stream.  With it, a launch whose last round of workgroups would leave most CUs idle (n workgroups on 256 CUs cost
 * ceil(n / 256) rounds: 896 -> 4 instead of 3.5) runs the tiles of that round as input-channel slices that fill the chip and adds the
 * slices in a fixed order (deterministic); without it the layer runs unsplit.  Not combined with PWC_CONV_SPLIT2. */
int64_t pwc_conv3x3_wino4_workspace_bytes(int B, int Cin, int H, int W, int Cout);
/* Inverse of `levels` nested PWC_CONV_SPLIT2 stores: x [B * 4^levels][C][h][w] (contiguous) -> y [B][C][h << levels][w << levels]
 * (dense planes, free batch stride); image index ((b*4 + s1)*4 + s2)... with s_i = 2 (y_i & 1) + (x_i & 1), coarsest split first. */
int pwc_lattice_unsplit_f32(const void *x, void *y, int B, int C, int h, int w, int levels, int64_t y_bstride, void *stream);

/* ---- image-space pre / post of the KITTI evaluation loop (reference inference_kitti.py:53-91,175-178,208-224; csrc/pwc_kitti.hip) ----
 * pwc_kitti_ingest_u8: uint8 RGB pairs [n][2][H][W][3] -> x float [n][6][Hp][Wp] (Hp, Wp = H, W rounded up to multiples of 64; free batch
 *   stride in elements, multiple of 4; 16-byte aligned): ToTensor (/ 255), (v - mean3[c]) / std3[c] (host pointers, read at the call),
 *   the two images concatenated along the channels, replicate padding at the bottom / right -- what the reference does with
 *   torchvision transforms, torch.cat and F.pad(mode="replicate") before the model.
 * pwc_flow_upsample_f32: the model's quarter-resolution flow [n][2][Hq][Wq] (free batch stride) -> out [n][2][out_h][out_w] (dense):
 *   crop to the top-left crop_h x crop_w, bilinear resize with align_corners = True (F.interpolate's arithmetic), u * (out_w / crop_w),
 *   v * (out_h / crop_h) -- `unpad` + `flow_resize` of the reference.  Neither allocates nor synchronises. */
int pwc_kitti_ingest_u8(const void *pairs_u8, void *x, int n, int H, int W, const float *mean3, const float *std3,
                        int64_t x_bstride, void *stream);
int pwc_flow_upsample_f32(const void *flow_q, void *out, int n, int Hq, int Wq, int crop_h, int crop_w, int out_h, int out_w,
                          int64_t q_bstride, void *stream);

/* Pillow-exact bilinear resize (ABI v13 additions, csrc/pwc_pil_resize.hip): transforms.Resize -> ToTensor -> Normalize of
 * train_pseudo.py:370-374 / train_fundamental.py:567-571 / inference.py:305-309 on 8-bit frames, and resize_flow of inference.py:162-190
 * on float planes.  Image.resize(..., BILINEAR) is a separable triangle filter whose support widens with the scale factor.  Per axis
 * with input length I and output length O the HOST makes, in IEEE double (opticalflow_amd/pil_resize.py coeff_tables / fixed_point):
 *   scale = I / O; fs = max(scale, 1); support = fs; ksize = 2 * ceil(support) + 1; for each output index xx:
 *   center = (xx + 0.5) * scale; first = max((int)(center - support + 0.5), 0); count = min((int)(center + support + 0.5), I) - first;
 *   w[t] = tri((t + first - center + 0.5) / fs), tri(v) = 1 - |v| for |v| < 1 else 0, divided by their sum in tap order when it is not 0.
 * bounds [O][2] int32 = (first, count); coefficients [O][ksize], taps past count zero: float64 w for planes, int32
 * k = (int)(w * 2^22 + 0.5) for frames.  All tables are DEVICE pointers; the kernels clamp what they hold so that no tap leaves the image.
 * pwc_pil_resize_frames_u8: frames uint8 [n][H][W][3] (interleaved RGB, dense) -> out_f32 planes of [h][w], and when out_u8 is not
 *   NULL the resized bytes [n][h][w][3].  sample = clip(0, 255, (2^21 + sum_t src[first + t] * k[t]) >> 22) in int32; the horizontal pass
 *   first, ROUNDED TO BYTES, the vertical pass on those bytes; out_f32 = lut768[c * 256 + byte] (float [3][256], device: ToTensor and
 *   Normalize tabulated by the caller).  Frame f is written to out_f32 + (f % out_group) * out_bstride + (f / out_group) * 3 * h * w
 *   (elements): out_group = n gives [n][3][h][w] with a free batch stride, out_group = n / 2 puts the second half of the frames
 *   into channels 3..5 of the first half's items (the [B][6][h][w] network input).
 * pwc_pil_resize_planes_f32: src float [n][c][in_h][in_w] (dense planes, free batch stride in elements) -> dst [n][c][out_h][out_w]
 *   (dense).  ss = 0.0; ss += (double)src[first + t] * w[t] in tap order, multiply and add separate; (float)ss; horizontal pass first
 *   with a float intermediate.  factors (device, float [c], may be NULL): dst = (float)ss * factors[channel] in float.
 * Two rules of Image.resize sit above the passes.  (1) It takes no pass on an axis whose length does not change, and copies when
 *   neither does.  pwc_pil_resize_planes_f32 does the same: with in_w == out_w its horizontal stage copies the sample, with
 *   in_h == out_h its vertical stage does, so -0.0, infinities and NaN stay where they are (the identity table would make +0.0 of
 *   -0.0 and NaN of an inf's or a NaN's neighbour).  pwc_pil_resize_frames_u8 applies the identity table, which is exact on bytes:
 *   its coefficient is 2^22 and (2^21 + v * 2^22) >> 22 == v.  (2) It takes the VERTICAL pass first when H > 100 * W and h < H.
 *   Both entry points (ops.pil_resize_frames, ops.pil_resize_planes) are single-order, horizontal first, whatever the sizes; a caller
 *   that wants Pillow's result for such a source makes two calls, (H, W) -> (h, W) and then (h, W) -> (h, w), each of which is a
 *   one-axis resize by rule (1), the bytes of the first going through out_u8.  opticalflow_amd/pil_resize.py (resize_frames,
 *   resize_planes, resize_flow, FrameIngest, infer_resized) does that.
 * One launch each (a workgroup resamples the source rows of its 16 x 64 output tile horizontally into LDS and takes the vertical pass
 * from there); neither allocates nor synchronises.  Supported: I <= 8 * O on both axes (a downscale of at most 8, ksize <= 17; any upscale), sizes <= 2^20;
 * beyond 8 only to an output shorter than a tile, as long as what a tile stages still fits: min(O, T) * ksize <= T * 17 coefficients
 * and at most 144 source rows (T = 16) / 522 source columns (T = 64) under it, e.g. 16 -> 1 or 29 -> 3 but not 129 -> 16
 * (pwc_pil_resize_supported: 1 / 0; pwc_pil_resize_ksize: the ksize of one axis, PWC_EINVAL when the pair is supported on neither axis).
 * PWC_EINVAL, nothing launched: a null pointer (out_u8 / factors may be NULL), non-positive sizes or out_group, an unsupported scale,
 * a ksize that disagrees with the sizes, a batch stride smaller than the tensor, n (frames) or n * c (planes) > 65535.  PWC_EALIGN,
 * nothing launched: out_f32 / src / dst / bounds / int32 coefficients / lut768 / factors not 4-byte, float64 coefficients not 8-byte aligned. */
int pwc_pil_resize_ksize(int in_size, int out_size);
int pwc_pil_resize_supported(int in_h, int in_w, int out_h, int out_w);
int pwc_pil_resize_frames_u8(const void *frames_u8, void *out_f32, void *out_u8, int n, int H, int W, int h, int w,
                             const int32_t *xbounds, const int32_t *xcoef, int xksize, const int32_t *ybounds, const int32_t *ycoef,
                             int yksize, const float *lut768, int64_t out_bstride, int out_group, void *stream);
int pwc_pil_resize_planes_f32(const void *src, void *dst, int n, int c, int in_h, int in_w, int out_h, int out_w,
                              const int32_t *xbounds, const double *xcoef, int xksize, const int32_t *ybounds, const double *ycoef,
                              int yksize, const float *factors, int64_t src_bstride, void *stream);

/* inference.py's resized flow, scored and / or encoded in the launch that resizes it (additions within ABI v13,
 * csrc/pwc_pil_resize.hip): resize_flow (inference.py:162-190), compute_epe / compute_fl (:105-159) and the array save_flow builds
 * (:266-282) for a batch, without a full-resolution float flow unless the caller asks for one.
 * src float [n][2][in_h][in_w] (dense planes, free batch stride in elements); tables and factors (float [2], may be NULL) exactly as
 * pwc_pil_resize_planes_f32 takes them with c = 2, the same supported range (pwc_pil_resize_supported), the same copy on an axis of
 * unchanged length and the same single order, horizontal first (for Pillow's vertical-first regime the caller runs the vertical pass
 * with pwc_pil_resize_planes_f32 and this entry point as the horizontal-only pass; opticalflow_amd/pil_resize.py eval_flow does).
 * Per output pixel (b, y, x), fp32 with no fused multiply-add:
 *   1. (pu, pv) = what pwc_pil_resize_planes_f32 writes there for channels 0 and 1: the two passes, then * factors[c] when factors
 *        is not NULL (no multiply otherwise);
 *   2. flow_out (may be NULL; float [n][2][out_h][out_w], dense): pu, pv, bit-identical to pwc_pil_resize_planes_f32;
 *   3. enc_out (may be NULL; uint16 [n][out_h][out_w][3], dense, 2-byte aligned and no more): eu = (uint16)(int)clamp(pu * 64.0f +
 *        32768.0f), ev alike; the cast truncates toward zero; clamp(t) = t < 0 or NaN -> 0, t > 65535 -> 65535.  The reference's
 *        (x * 64.0 + 2**15).astype(np.uint16) is the same float32 expression and wraps modulo 2^16 out of range, where the C cast
 *        is undefined: the clamp is a stated deviation for |flow| >= 512 px (kitti.encode_flow_rgb16 clips likewise).
 *        enc_order 0 (save_flow's own order): the samples {1, ev, eu};  enc_order 1 (the devkit's R, G, B = u, v, valid; what
 *        kitti.write_png16_rgb / read_png16_rgb and pwc_kitti_score use): {eu, ev, 1};
 *   4. score, when gt is not NULL.  gt_kind 0: float planes [n][2][out_h][out_w] with valid uint8 [n][out_h][out_w] (non-zero =
 *        valid) or NULL (all valid);  gt_kind 1: uint16 [n][out_h][out_w][3] as R, G, B = u, v, valid, decoded
 *        ((float)s - 32768.f) / 64.f, valid = (B != 0);  gt_kind 2: the same samples in the reference's own order {valid, v, u}
 *        (inference.py:89-102).  valid must be NULL with kinds 1 and 2.  Then as pwc_kitti_score step 3:
 *        du = pu - gu; dv alike; epe = sqrtf(du*du + dv*dv); mag = sqrtf(gu*gu + gv*gv); OUTLIER when epe > fmaxf(3.0f, 0.05f * mag);
 *        per sample {fp64 sum of the fp32 epe over valid pixels, int64 #valid, int64 #valid outliers}.
 * out (device, float [n][2], needed with gt): {(float)(sum / #valid), (float)(100.0 * #outliers / #valid)}, both NaN when #valid == 0
 * (inference.py reports 0.0 there; opticalflow_amd/inference_eval.py does that on the host from the raw counts).
 * workspace (needed with gt): device, 8-byte aligned, pwc_pil_flow_eval_workspace_bytes(n, out_h, out_w) = 24 * n * (1 + tiles per
 * sample) bytes (-1 for a non-positive size).  Each 16 x 64 tile leaves its three totals there, summed in a fixed tree order, and one
 * final workgroup per sample adds that sample's tiles in order: no atomics, bit-reproducible, no host synchronisation.  After the
 * launch its first 24 n bytes hold the raw totals, [n][3] 8-byte words: fp64 sum, int64 #valid, int64 #outliers.
 * One workgroup resizes BOTH channels of its 16 x 64 tile: channel u is staged in LDS and finished into registers, then the same LDS
 * stages channel v.  One launch (two with gt); neither allocates nor synchronises; can be captured in a graph.
 * PWC_EINVAL, nothing launched: null src or table; none of gt / flow_out / enc_out; gt without workspace or out; non-positive sizes; an
 * unsupported scale; a ksize that disagrees with the sizes; src_bstride < 2*in_h*in_w; gt_kind outside 0..2 (with gt); enc_order
 * outside 0..1 (with enc_out); valid != NULL without gt or with gt_kind 1 / 2; n > 65535 (indexing is 64-bit throughout); a workspace that
 * is too small.  PWC_EALIGN, nothing launched: workspace or coefficients not 8-byte, src / flow_out / out / float gt / bounds /
 * factors not 4-byte, enc_out / uint16 gt not 2-byte aligned. */
int64_t pwc_pil_flow_eval_workspace_bytes(int n, int out_h, int out_w);
int pwc_pil_flow_eval(const void *src, int n, int in_h, int in_w, int out_h, int out_w, const int32_t *xbounds, const double *xcoef,
                      int xksize, const int32_t *ybounds, const double *ycoef, int yksize, const float *factors, int64_t src_bstride,
                      const void *gt /* may be NULL */, int gt_kind, const void *valid /* may be NULL */,
                      void *flow_out /* may be NULL */, void *enc_out /* may be NULL */, int enc_order, void *workspace,
                      int64_t workspace_bytes, void *out /* float [n][2] */, void *stream);

/* cv2.resize-exact INTER_LINEAR resize (ABI v13 additions, csrc/pwc_cv_resize.hip): the two cv2.resize calls around the model in
 * script_pwc.py:43-83 and topview.py:79-119 (compute_flow), with what surrounds them -- channel flip, / 255, HWC -> CHW, stacking on
 * the way in; the gain (x 20 in script_pwc.py), the resize and the u / v rescale on the way out.  "Exact" means equal to this project's
 * statement of OpenCV's published algorithm (opticalflow_amd/harness.py, pinned by tests/test_harness.py); cv2 parity unpinned.  Per
 * axis with input length I and output length O the HOST makes (opticalflow_amd/cv_resize.py axis_table):
 *   scale = 1.0 / ((double)O / (double)I); for each output index d: fx = (float)((d + 0.5) * scale - 0.5); s0 = floor(fx); fx -= s0;
 *   s0 < 0 -> (0, fx = 0); s0 >= I - 1 -> (I - 1, fx = 0).
 * xs0 / ys0 are int32 [O] (first tap), xfx / yfy float [O] (weight of the second tap, s1 = min(s0 + 1, I - 1)).  All tables are DEVICE
 * pointers; the kernels clamp s0 into [0, I), so no tap leaves the image whatever a table holds.
 * pwc_cv_resize_frames_u8: frames uint8 [n][H][W][3] (interleaved, dense) -> out_f32 planes of [h][w].  a0 = cvRound((1.f - fx) * 2048),
 *   a1 = cvRound(fx * 2048) (round half to even, each on its own: their sum may be 2047 or 2049), b0 / b1 alike from fy;
 *   D = S[s0] * a0 + S[s1] * a1 in int32 on source rows y0 and y1; byte = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2;
 *   out_f32 = lut768[c_out * 256 + byte] with c_out = flip_channels ? 2 - c : c (float [3][256], device: / 255 and any normalisation
 *   tabulated by the caller, indexed by the OUTPUT channel).  Frame f is written to
 *   out_f32 + (f % out_group) * out_bstride + (f / out_group) * 3 * h * w (elements), as pwc_pil_resize_frames_u8 does: out_group = n
 *   gives [n][3][h][w] with a free batch stride; pairs [n][2][H][W][3] taken as 2n frames with out_group = 2n and
 *   out_bstride = 3 * h * w fill a dense [n][6][h][w] network input in one launch.  H == h && W == w needs no special case: weight 2048 is
 *   exact on bytes.
 * pwc_cv_resize_flow_f32: src float [n][2][in_h][in_w] (dense planes, free batch stride in elements) -> dst [n][2][out_h][out_w], or
 *   [n][out_h][out_w][2] when hwc (dense).  In float32, every product and sum rounded (no fused multiply-add): t = src * gain;
 *   row = t[s0] * (1.f - fx) + t[s1] * fx; val = row[y0] * (1.f - fy) + row[y1] * fy; dst = val * (channel 0 ? fu : fv).  When both sizes
 *   are equal cv2 copies: dst = (src * gain) * f, so -0.0, infinities and NaN stay where they are.
 * One launch each, a direct four-tap gather: a thread owns four consecutive outputs of a row in every channel and stores 16 bytes per
 * plane where out_w % 4 == 0 and the output is 16-byte aligned (frames: out_bstride % 4 == 0 too), single floats otherwise.  Neither
 * allocates nor synchronises; both can be captured in a graph.
 * PWC_EINVAL, nothing launched: a null pointer, a size outside 1..2^20, non-positive n or out_group, a batch stride smaller than the
 * tensor, n > 65535.  PWC_EALIGN, nothing launched: out_f32 / src / dst / a table not 4-byte aligned. */
int pwc_cv_resize_frames_u8(const void *frames_u8, void *out_f32, int n, int H, int W, int h, int w, const int32_t *xs0,
                            const float *xfx, const int32_t *ys0, const float *yfy, const float *lut768, int flip_channels,
                            int64_t out_bstride, int out_group, void *stream);
int pwc_cv_resize_flow_f32(const void *src, void *dst, int n, int in_h, int in_w, int out_h, int out_w, const int32_t *xs0,
                           const float *xfx, const int32_t *ys0, const float *yfy, float gain, float fu, float fv, int hwc,
                           int64_t src_bstride, void *stream);

/* cv2.warpPerspective-exact warp of 8-bit frames (ABI v13 addition, csrc/pwc_cv_warp.hip): the cv2.warpPerspective(frame, M,
 * (width, height)) of topview.py:218,232 with the script's defaults INTER_LINEAR, BORDER_CONSTANT, border value 0.  "Exact" means
 * equal to this project's statement of OpenCV's published algorithm (imgproc's warpPerspective plus the 8-bit bilinear remap; as
 * NumPy in tests/cv_warp_oracle.py); cv2 parity unpinned.  Also unpinned: how OpenCV's int16 weight table stores the single weight
 * 32768 at ax = ay = 0; it is taken as 32768, so an identity warp returns the image.
 * src uint8 [n][H][W][3], dst uint8 [n][h][w][3], both dense frames with free batch strides in BYTES.  mat9: DEVICE pointer to the
 * INVERSE map Mi (destination -> source), 9 doubles row-major per frame; frame f uses mat9 + f * mat_stride (0: one matrix for all
 * frames, 9: one each).  The host inverts (opticalflow_amd/cv_warp.py invert3x3: OpenCV's closed 3x3 form, determinant by cofactor
 * expansion along the first row, d = 1.0 / det, each adjugate entry times d).
 * Coordinates, float64, every product and sum rounded separately (no fused multiply-add), for destination pixel (x, y):
 *   bh0 = min(16, h); bw0 = min(1024 / bh0, w); xb = (x / bw0) * bw0; x1 = x - xb   (OpenCV's block origin and offset; integer)
 *   X0 = (Mi[0]*xb + Mi[1]*y) + Mi[2];  Y0 = (Mi[3]*xb + Mi[4]*y) + Mi[5];  W0 = (Mi[6]*xb + Mi[7]*y) + Mi[8]
 *   Wd = W0 + Mi[6]*x1;  Wd = (Wd != 0) ? 32.0 / Wd : 0.0                           (IEEE double division)
 *   fX = max(-2147483648.0, min(2147483647.0, (X0 + Mi[0]*x1) * Wd));  fY alike with Y0 and Mi[3]
 *        (std::min / std::max as OpenCV writes them: a NaN product becomes 2147483647.0)
 *   X = cvRound(fX) (round half to even, int32);  sx = clamp(X >> 5, -32768, 32767) (arithmetic shift);  ax = X & 31;  Y, sy, ay alike
 * Pixel, integer: over the four taps (sx + dx, sy + dy), dx, dy in {0, 1}, with wx in {32 - ax, ax} and wy in {32 - ay, ay}, a tap
 * outside [0, W) x [0, H) contributing 0: per channel D = (sum wx * wy * S_tap + 512) >> 10.  This is OpenCV's 15-bit table form
 * (sum w15 * S + 16384) >> 15 with w15 = 32 * wx * wy, exact for bilinear weights at 1 / 32 steps.
 * One launch for the n frames, a direct gather: a thread owns four consecutive destination pixels of one row and stores them as three
 * dwords where w % 4 == 0 and dst and dst_bstride are 4-byte aligned, as bytes otherwise.  No tap address leaves its frame.  Neither
 * allocates nor synchronises; can be captured in a graph.
 * PWC_EINVAL, nothing launched: a null pointer, a size outside 1..32767 (the statement's int16 coordinate range), n outside 1..65535,
 * mat_stride not 0 or 9, a batch stride smaller than its frame.  PWC_EALIGN, nothing launched: mat9 not 8-byte aligned. */
int pwc_cv_warp_perspective_u8(const void *src_u8, void *dst_u8, int n, int H, int W, int h, int w, const double *mat9, int mat_stride,
                               int64_t src_bstride, int64_t dst_bstride, void *stream);

/* Raw video frames -> network input (ABI v13 addition, csrc/pwc_video.hip): frame_to_tensor + pad_to_multiple_of_64 of
 * pwc_extract_flow_video.py:27-42 as one kernel (host mirror: opticalflow_amd/video.py frame_to_tensor + kitti.pad_to_64; as NumPy in
 * tests/video_ingest_oracle.py).
 * frames_u8 uint8 [n][H][W][3] (interleaved, dense frames) with a free batch stride in BYTES: a frame may be one slot of a larger
 * buffer, and since rows are 3 * W bytes NO alignment of the source is assumed.  x float [n][3][Hp][Wp] planes, Hp / Wp = H / W rounded
 * up to multiples of 64, batch stride in ELEMENTS.
 *   x[f][c][y][x'] = (float)S[f][min(y, H - 1)][min(x', W - 1)][bgr ? 2 - c : c] / 255.0f
 * as an IEEE float32 division, correctly rounded (a multiplication by 1 / 255 differs for 126 of the 256 byte values); the clamped
 * source coordinate is the replicate padding at the bottom and right.
 * One launch for the n frames: a thread owns four consecutive output columns of one row in the three planes and stores 16 bytes per
 * plane; its twelve source bytes are read as three dwords when they start on a dword boundary inside the row, as bytes otherwise.
 * 64-bit indexing throughout.  Neither allocates nor synchronises; can be captured in a graph.
 * PWC_EINVAL, nothing launched: a null pointer, n < 1, H or W outside 1..2^20, src_bstride < 3*H*W, x_bstride < 3*Hp*Wp.
 * PWC_EALIGN, nothing launched: x not 16-byte aligned or x_bstride not a multiple of 4. */
int pwc_video_ingest_u8(const void *frames_u8, void *x, int n, int H, int W, int bgr, int64_t src_bstride, int64_t x_bstride,
                        void *stream);

/* KITTI scoring on the device (ABI v13 additions, csrc/pwc_kitti_score.hip): EPE and Fl-all of inference_kitti.py:94-128
 * (epe_metric / fl_all_metric) straight from the network's quarter-resolution flow, nothing image-sized written unless asked for.
 * flow_q [n][2][Hq][Wq] f32 (dense planes, batch stride in elements).  Per pixel (b, y, x) of the out_h x out_w grid, in fp32 with
 * no fused multiply-add:
 *   1. pred = what pwc_flow_upsample_f32(flow_q, crop_h, crop_w, out_h, out_w) writes at that pixel -- the same crop, rh / rw / su /
 *        sv and expression order (one shared device function, csrc/pwc_flow_up.h); with (crop_h, crop_w) == (out_h, out_w) every
 *        interpolation weight is exactly 1 or 0 and the scale is 1, so the value is the field's own;
 *   2. ground truth, gt_kind 0: gt = float planes [n][2][out_h][out_w], valid = uint8 [n][out_h][out_w] (non-zero = valid) or NULL
 *        (every pixel valid);  gt_kind 1: gt = the KITTI PNG samples themselves, uint16 [n][out_h][out_w][3] in R, G, B order:
 *        u = ((float)R - 32768.f) / 64.f, v alike from G, valid = (B != 0) (load_flow_kitti_png, inference_kitti.py:23-52); valid
 *        must be NULL;
 *   3. du = pred.u - gt.u;  dv alike;  epe = sqrtf(du*du + dv*dv);  mag = sqrtf(gu*gu + gv*gv);
 *        the pixel is an OUTLIER when epe > fmaxf(3.0f, 0.05f * mag)  (inference.py:129-159 compute_fl writes the same predicate as
 *        (epe > 3) & (epe > 0.05 * mag));
 *   4. per sample b: {fp64 sum of epe over valid pixels (each fp32 epe added in fp64), int64 #valid, int64 #valid outliers}.
 * out (device, float [n][2]): out[b] = {(float)(sum / #valid), (float)(100.0 * #outliers / #valid)}; both NaN when #valid == 0
 * (the reference's np.nan; inference.py returns 0.0 there -- a caller who wants that reads the raw counts).  Each 16 x 64 tile leaves
 * its three totals in the workspace, summed in a fixed tree order, and one final workgroup per sample adds that sample's tiles in
 * order: no atomics, bit-reproducible, no host synchronisation.
 * flow_out: NULL, or float [n][2][out_h][out_w] (dense) that also receives the full-resolution flow, bit-identical to
 * pwc_flow_upsample_f32.
 * workspace: device, 8-byte aligned, pwc_kitti_score_workspace_bytes(n, out_h, out_w) = 24 * n * (1 + tiles per sample) bytes (-1
 * for a non-positive size).  After the launch its first 24 n bytes hold the raw totals, [n][3] 8-byte words: fp64 sum, int64 #valid,
 * int64 #outliers.
 * PWC_EINVAL, nothing launched: null flow_q / gt / workspace / out, non-positive sizes, crop_h > Hq or crop_w > Wq, q_bstride <
 * 2*Hq*Wq, gt_kind not 0 or 1, valid != NULL with gt_kind 1, n*2*out_h*out_w >= 2^31, n > 65535, out_h > 16 * 65535, a workspace
 * that is too small.  PWC_EALIGN, nothing launched: a workspace not 8-byte aligned, flow_q / flow_out / out / float gt not 4-byte
 * aligned, uint16 gt not 2-byte aligned. */
int64_t pwc_kitti_score_workspace_bytes(int n, int out_h, int out_w);
int pwc_kitti_score(const void *flow_q, int n, int Hq, int Wq, int crop_h, int crop_w, int out_h, int out_w,
                    int64_t q_bstride,
                    const void *gt, int gt_kind, const void *valid,
                    void *flow_out /* may be NULL */, void *workspace, int64_t workspace_bytes,
                    void *out /* float [n][2] */, void *stream);

/* Flow-comparison report on the device (additions within ABI v13, csrc/pwc_flow_compare.hip): compare_flows and print_flow_stats of
 * onnx_pth_compare.py:133-201, :225-230 in one launch pair.  a (the reference side, "pth") and b are f32 [n][2][H][W]; each sample's
 * [2][H][W] is contiguous, the batch strides (in elements, >= 2*H*W) are free and separate.  Per pixel, fp32 with no fused
 * multiply-add, square root correctly rounded:
 *   du = a_u - b_u;  dv = a_v - b_v;  epe = sqrtf(du*du + dv*dv)      -- bit for bit the reference's float32 np.linalg.norm(a - b, axis=-1)
 * Per scalar (2 per pixel) the f32 values d = a - b, a, b are widened to fp64 and d*d, |d|, a*a, b*b, |a|, a, b, a*b are added in
 * fp64; epe is added in fp64 per pixel.  max |d|, max epe and min / max of a and of b are exact f32 reductions; count_k is the
 * number of pixels with epe <= taus[k] (inclusive, f32 comparison).  taus: HOST array of ntau (1..PWC_FLOW_COMPARE_MAX_TAUS) finite
 * non-negative floats, read during the call and passed to the kernel by value.
 * out (device, 8-byte aligned): double [n + 1][PWC_FLOW_COMPARE_FIELDS].  Row s < n is sample s; row n is the whole batch, which is
 * the reference called on the samples stacked along H.  With N = 2*H*W*(samples in the row) and P = N / 2, all formed in fp64 from
 * the totals:
 *   L2 = sqrt(S d^2)   MAE = S|d| / N   REL_L2 = L2 / (sqrt(S a^2) + 1e-8)   REL_MAE = MAE / (S|a| / N + 1e-8)
 *   COSINE = S ab / (sqrt(S a^2) * sqrt(S b^2) + 1e-8)
 *   PEARSON = (S ab - S a * S b / N) / sqrt((S a^2 - (S a)^2 / N) * (S b^2 - (S b)^2 / N)), clipped to [-1, 1] as np.corrcoef does;
 *             NaN when min == max for either field (np.corrcoef's NaN; the exact test keeps rounding from turning it into noise)
 *   EPE_MEAN = S epe / P   AGREE_k = (double)count_k / P * 100.0 (the reference's (vec_diff <= tau).mean() * 100.0 bit for bit;
 *             NaN for k >= ntau)
 *   MEAN_A = S a / N, STD_A = sqrt(max(S a^2 / N - MEAN_A^2, 0)), exactly 0 when min == max; MEAN_B / STD_B alike (population std)
 * NaN / Inf inputs are not special-cased: the sums carry them as IEEE arithmetic dictates, epe <= tau is false for a NaN epe, and
 * the extrema come from fmaxf, which returns the other operand when one is NaN (np.max would return NaN).
 * epe_map: NULL, or float [n][H][W] (dense) that receives the per-pixel epe; the record is the same bits with and without it.
 * Each 32 x 128 tile leaves its totals (fixed tree order) in the workspace; the finish kernel's workgroup s < n adds the tiles of
 * sample s in tile order, workgroup n adds every tile in (sample, tile) order: no atomics, bit-reproducible, no allocation, no host
 * synchronisation, no host callback -- the call can be captured in a graph (taus are captured by value).
 * workspace: device, 8-byte aligned, pwc_flow_compare_workspace_bytes(n, H, W) = 128 * n * tiles per sample bytes (-1 for a
 * non-positive size).
 * PWC_EINVAL, nothing launched: a null a / b / taus / workspace / out, non-positive sizes, ntau outside 1..8, a tau that is negative,
 * NaN or infinite, n*2*H*W >= 2^31, n > 65535, H > 32 * 65535, a batch stride < 2*H*W, a workspace that is too small, workspace / out
 * not 8-byte aligned, a / b / epe_map not 4-byte aligned. */
#define PWC_FLOW_COMPARE_MAX_TAUS 8
#define PWC_FLOW_COMPARE_FIELDS 44
#define PWC_FC_N 0         /* scalars in the row, as a double */
#define PWC_FC_P 1         /* pixels in the row */
#define PWC_FC_SUM_D2 2
#define PWC_FC_SUM_ABS_D 3
#define PWC_FC_SUM_A2 4
#define PWC_FC_SUM_B2 5
#define PWC_FC_SUM_ABS_A 6
#define PWC_FC_SUM_A 7
#define PWC_FC_SUM_B 8
#define PWC_FC_SUM_AB 9
#define PWC_FC_SUM_EPE 10
#define PWC_FC_MAX_ABS 11  /* "Max abs diff" */
#define PWC_FC_EPE_MAX 12
#define PWC_FC_MIN_A 13
#define PWC_FC_MAX_A 14
#define PWC_FC_MIN_B 15
#define PWC_FC_MAX_B 16
#define PWC_FC_COUNT0 17   /* 17..24: count_k as a double (exact), 0 for k >= ntau */
#define PWC_FC_L2 25
#define PWC_FC_MAE 26
#define PWC_FC_REL_L2 27
#define PWC_FC_REL_MAE 28
#define PWC_FC_PEARSON 29
#define PWC_FC_COSINE 30
#define PWC_FC_EPE_MEAN 31
#define PWC_FC_AGREE0 32   /* 32..39: agreement in percent */
#define PWC_FC_MEAN_A 40
#define PWC_FC_STD_A 41
#define PWC_FC_MEAN_B 42
#define PWC_FC_STD_B 43
int64_t pwc_flow_compare_workspace_bytes(int n, int H, int W);
int pwc_flow_compare(const void *a, const void *b, int n, int H, int W, int64_t a_bstride, int64_t b_bstride,
                     const float *taus /* host */, int ntau, void *epe_map /* may be NULL */,
                     void *workspace, int64_t workspace_bytes,
                     void *out /* double [n + 1][PWC_FLOW_COMPARE_FIELDS] */, void *stream);

/* Flow pictures on the device (additions within ABI v13, csrc/pwc_flowviz.hip).  All three read the top-left crop_h x crop_w of
 * flow [n][2][Hq][Wq] f32 (dense planes, batch stride in elements): the reference colours and draws the cropped quarter-resolution
 * flow.  fp32 with no fused multiply-add, divisions and square roots correctly rounded; no atomics, so every output is
 * bit-reproducible; nothing allocates or synchronises.  Behaviour on NaN / infinite flow is undefined, as in the reference.
 *
 * pwc_flow_stats: per sample the 16-byte record rec[b] = {float max radius, int32 count, float mean u, float mean v}:
 *   max radius = max over the crop of sqrtf(u*u + v*v) of (u, v) AFTER the optional clip (use_clip != 0, flow_to_color lines 65-69):
 *        rad = sqrtf(u*u + v*v);  k = clip_flow / fmaxf(fmaxf(rad, 1e-5f), clip_flow);  u = u * k;  v = v * k;
 *   count / means over the pixels whose UNCLIPPED sqrtf(u*u + v*v) > threshold (calculate_dominant_direction): each fp32 u and v is
 *        added in fp64, mean = (float)(sum / count); both means are 0 when count == 0 (the reference returns [0, 0]).
 *   Each 16 x 64 tile leaves {fp64 sum u, fp64 sum v, int64 count, fp32 max} in the workspace, summed in a fixed tree order, and one
 *   final workgroup per sample adds that sample's tiles in tile order.  workspace: device, 8-byte aligned,
 *   pwc_flow_stats_workspace_bytes(n, crop_h, crop_w) = 32 * n * tiles per sample bytes (-1 for a non-positive size).
 * pwc_flow_color: out uint8 [n][crop_h][crop_w][3], R G B, contiguous, at ANY byte address (3 bytes per pixel: a sample starts
 *   unaligned in general); only those n*crop_h*crop_w*3 bytes are written.  rec is the record of pwc_flow_stats for the same flow, crop
 *   and clip (read on the device).  Per pixel, flow_to_color operation for operation, with (u, v) after the same optional clip:
 *        rad = sqrtf(u*u + v*v);  ang = atan2f(-v, -u) / (float)pi;  fk = (ang + 1.f) / 2.f * 54.f + 1.f;
 *        k0 = ((int)floorf(fk) - 1) % 55;  k1 = (k0 + 1) % 55;  f = fk - floorf(fk);
 *        col = (1.f - f) * wheel[k0][c] + f * wheel[k1][c]      wheel = the 55-entry make_colorwheel (RY 15, YG 6, GC 4, CB 11, BM 13,
 *                                                               MR 6) as (float)entry / 255.f
 *        rn = clip(rad / (rec[b].max + 1e-5f), 0, 1);  col = 1.f - rn * (1.f - col);  out = (uint8)(clip(col, 0, 1) * 255.f)  (truncation)
 *   The wheel is NOT continuous where the angle wraps (54 intervals over 55 entries): (u > 0, v = +0.0) gives (255, 0, 0), (u > 0,
 *   v = -0.0) gives (255, 0, 43); the sign of a zero reaches atan2f unchanged.  1 - f is exact (f is the fraction of an fp32 fk >= 1), so
 *   a channel whose two wheel entries are 255 is exactly 255 before the attenuation.
 * pwc_flow_quiver: the arrow grid at y = 0, step, ... < frame_h and x = 0, step, ... < frame_w (Gy = ceil(frame_h / step), Gx alike):
 *        (dx, dy) = value of cv2.resize(plane, (frame_w, frame_h)) (INTER_LINEAR, float path: geometry in double then float,
 *                   horizontal pass, then vertical pass) at (y, x), times (vec_sx, vec_sy); when (crop_h, crop_w) == (frame_h,
 *                   frame_w) the flow's own value (cv::resize copies);
 *        keep  = !(sqrtf(dx*dx + dy*dy) < min_mag);
 *        tip   = ((float)x + dx * gain, (float)y + dy * gain) to int: tip_rule 0 = round half to even (int(round(.)) of
 *                create_quiver_frame, gain = 1 / max(scale, 1e-6)), tip_rule 1 = toward zero (int(.) of draw_flow_arrows, gain = scale);
 *        aligned = 1 when dominant is NULL or the zero vector, else acosf(clip(dot(unit(dx, dy), unit(dominant)), -1, 1)) * 180.f /
 *                (float)pi < angle_threshold (draw_flow_arrows lines 157-171; 0 for a zero (dx, dy)).
 *   dominant: NULL, or device floats, sample b's (u, v) at dominant[b * dom_stride] and the next float (dom_stride 4 and rec + 2 reads
 *   the means of pwc_flow_stats).  vec float [n][Gy][Gx][2], tip int32 [n][Gy][Gx][2] (x, y), flags uint8 [n][Gy][Gx] (bit 0 keep,
 *   bit 1 aligned).
 * PWC_EINVAL, nothing launched: a null pointer, non-positive sizes, crop_h > Hq or crop_w > Wq, bstride < 2*Hq*Wq, n*crop_h*crop_w*3
 * >= 2^31, 2*Hq*Wq >= 2^31, n > 65535, use_clip with clip_flow <= 0, step < 1, tip_rule not 0 or 1, dom_stride < 2, more than 65535
 * tile or grid rows, a workspace that is too small.  PWC_EALIGN, nothing launched: flow / rec / dominant not 4-byte aligned, workspace /
 * vec / tip not 8-byte aligned. */
int64_t pwc_flow_stats_workspace_bytes(int n, int crop_h, int crop_w);
int pwc_flow_stats(const void *flow, int n, int Hq, int Wq, int crop_h, int crop_w, int64_t bstride, int use_clip, float clip_flow,
                   float threshold, void *workspace, int64_t workspace_bytes, void *rec /* [n][4] 4-byte words */, void *stream);
int pwc_flow_color(const void *flow, int n, int Hq, int Wq, int crop_h, int crop_w, int64_t bstride, int use_clip, float clip_flow,
                   const void *rec, void *out /* uint8 [n][crop_h][crop_w][3] */, void *stream);
int pwc_flow_quiver(const void *flow, int n, int Hq, int Wq, int crop_h, int crop_w, int64_t bstride, int frame_h, int frame_w,
                    int step, float vec_sx, float vec_sy, float gain, int tip_rule, float min_mag,
                    const void *dominant /* may be NULL */, int64_t dom_stride, float angle_threshold,
                    void *vec, void *tip, void *flags, void *stream);

/* Vanishing point of a flow field (additions within ABI v13, csrc/pwc_vanishing.hip): estimate_vanishing_point_from_flow of
 * pwc_extract_flow_video_vanishpoint.py:93-255 per frame, from vec float [n][gy][gx][2] as pwc_flow_quiver writes it ((dx, dy) in frame
 * pixels at x = gx*step, y = gy*step; gy = ceil(frame_h / step), gx alike).  fp64 throughout, no fused multiply-add.
 *   select   dx, dy widened; mag = hypot(dx, dy); a cell is kept when mag >= min_mag AND mag is finite; N = number kept.  This departs
 *            from the reference, whose `mag < min_mag: continue` keeps a NaN magnitude (which then poisons its median and costs it the
 *            refinement) and an infinite one: here a cell with a NaN or an infinite component counts as a cell below min_mag, and
 *            the frame is answered from the others.  N <= max_points: all kept cells
 *            in row-major order.  N > max_points: the kept cells in the sequence of `order` (int32, a permutation of the gy*gx cells),
 *            the first max_points of them, in that sequence.  An `order` that is no permutation is read as it stands: an entry
 *            outside 0 .. gy*gx-1 or naming a cell that is not kept is skipped; an entry that repeats an earlier one selects its
 *            cell AGAIN (nothing records what was selected; the two copies are parallel, so they add no pair of their own, but each
 *            pairs with every other line); and when the table names fewer than max_points kept cells, N used is that number.
 *            N used < 5: status 2.
 *   pairs    for i < j in the selected order, with (dxn, dyn) = (dx / mag, dy / mag):
 *                 denom = d1x*d2y - d1y*d2x;  skipped when fabs(denom) < 1e-6;
 *                 t1 = ((p2x - p1x)*d2y - (p2y - p1y)*d2x) / denom;  ix = p1x + t1*d1x;  iy = p1y + t1*d1y;
 *            kept when -0.5*W <= ix <= 1.5*W and -0.5*H <= iy <= 1.5*H; fewer than min_pairs kept: status 3.
 *   votes    np.histogram2d's bins: edges e[k] = k*((hi - lo)/grid) + lo for k < grid and e[grid] = hi, a value in the bin with
 *            e[k] <= v < e[k+1], v == hi in the last one.  A pair adds llrint((mag_i / M)*(mag_j / M) * 2^40), M the largest selected
 *            magnitude of the frame, with a 64-bit integer atomic: the histogram has the same bits on every run.
 *   best     arg-max over gx*grid + gy, the lowest index on a tie; not positive: status 4.  centre = 0.5*(e[g] + e[g+1]) per axis;
 *            prob = best / (total + 1e-9 * 2^40 / M^2), the reference's best / (total + 1e-9) in the scaled units.
 *   refine   n = (-dyn, dxn), c = nx*x + ny*y, dist = fabs(nx*cxf + ny*cyf - c) with the centre rounded to float and widened (the
 *            reference's float32 candidate); median of the N distances (mean of the two middle ones for even N); inliers are
 *            dist < 3*median + 1e-6.  With >= 5 inliers the 2x2 normal equations of n . (v - centre) = c - n . centre over the
 *            inliers, summed in a fixed order; det not finite or <= 1e-12 * trace^2, or < 5 inliers: the centre stands, status 1.
 * out_vp double [n][5] = (vx, vy, prob, centre x, centre y), (NaN, NaN, 0, NaN, NaN) for status >= 2; out_info int32 [n][6] = (status,
 * N used, pairs kept, best gx, best gy, inliers), best = -1 and inliers = 0 for status >= 2, pairs = 0 for status 2.
 * workspace: device, 8-byte aligned, pwc_vanishing_workspace_bytes(n, gy, gx, grid) = n * (24 + 8*grid^2 + 4096) bytes (-1 for a
 * geometry the call refuses).  Three launches on `stream`, nothing allocated, no synchronisation.
 * PWC_EINVAL, nothing launched: a null vec / out_vp / out_info / workspace, step < 1, non-positive sizes, n > 65535, more than 65536
 * cells, gy / gx not the grid of the frame, grid outside 2..128, max_points outside 5..1024, gy*gx > max_points with a NULL order, a
 * workspace that is too small.  PWC_EALIGN: vec / out_vp / workspace not 8-byte aligned, order / out_info not 4-byte aligned. */
int64_t pwc_vanishing_workspace_bytes(int n, int gy, int gx, int grid);
int pwc_vanishing_point(const void *vec, int n, int gy, int gx, int frame_h, int frame_w, int step, double min_mag, int max_points,
                        int grid, int min_pairs, const void *order_or_null /* int32 [gy*gx] */, void *out_vp /* double [n][5] */,
                        void *out_info /* int32 [n][6] */, void *workspace, int64_t workspace_bytes, void *stream);

/* Training batches of KITTI on the device (addition within ABI v13, csrc/pwc_augment.hip): the "reduced augmentation" (small rotation /
 * zoom / squeeze affine), the random crop and the horizontal flip of KittiFlowDataset (data_processing_or.py:228-294) in one launch,
 * from the raw uint8 frames and the ground truth to the (x, flow, valid) train_one_epoch consumes.  Only the crop_h x crop_w window is
 * computed.  cv2.warpAffine (INTER_LINEAR, BORDER_REFLECT_101) is DEFINED here by a restatement of OpenCV's classic fixed-point path
 * (the one OpenCV used through 4.10); parity against an actual cv2 build is UNPINNED (cv2 is not available where this was written).
 * Everything is integer arithmetic, or fp32 / fp64 with the expression order below and no fused multiply-add, so the result is
 * bit-reproducible and bit-identical to tests/augment_oracle.py.
 *
 * Sources sit in fixed slots of Hs x Ws (the batch's largest size); sample b is stored densely in the top of its slot with ITS OWN ROW
 * STRIDE W_b (KITTI frames are 370-376 x 1224-1242):
 *   frames  uint8 [n][2][Hs*Ws*3], pixel (y, x) channel c of frame f of sample b at ((b*2 + f)*Hs*Ws + y*W_b + x)*3 + c, R G B
 *   gt      gt_kind 0: float [n][2][Hs*Ws] (u plane, v plane), element y*W_b + x; valid = uint8 [n][Hs*Ws] (non-zero = valid) or NULL
 *           (every pixel valid);  gt_kind 1: the KITTI PNG samples uint16 [n][Hs*Ws][3] in R, G, B order, decoded per tap as
 *           u = ((float)R - 32768.f) / 64.f, v likewise from G, valid = (B != 0); valid must be NULL
 *   params  DEVICE buffer, 8-byte aligned, one pwc_augment_params record (88 bytes) per sample:
 *           m[6]  the INVERTED 2x3 matrix in fp64, as cv::warpAffine inverts the float32 M = [A | t] after converting it to double:
 *                 D = M0*M4 - M1*M3; D = D ? 1/D : 0; A11 = M4*D; A22 = M0*D; M0 = A11; M1 *= -D; M3 *= -D; M4 = A22;
 *                 b1 = -M0*M2 - M1*M5; b2 = -M3*M2 - M4*M5; M2 = b1; M5 = b2
 *           a[4]  the float32 linear part A = {A00, A01, A10, A11} of the forward matrix (applied to the flow vectors)
 *           y0, x0  crop origin in the (warped) frame;  h, w = H_b, W_b the sample's own size;  warp, flip  flags (non-zero = on)
 *   x float [n][6][crop_h][crop_w] (channels 0-2 frame 1, 3-5 frame 2, in [0, 1]), flow float [n][2][crop_h][crop_w],
 *   valid_out float [n][1][crop_h][crop_w] (0 / 1), status int32 [n]; all dense.
 * Per output pixel (y', x') of sample b:
 *   xs = flip ? crop_w - 1 - x' : x';  (Y, X) = (y0 + y', x0 + xs)      the reference crops after warping and flips after cropping
 *   warp == 0: the sources are read at (Y, X):  x = (float)byte / 255.f, flow = the (decoded) ground truth, valid = (source != 0)
 *   warp != 0: fp64 and int32, rint = round half to even (OpenCV's saturate_cast<int>(double)):
 *        ad = rint(M0 * X * 1024);  bd = rint(M3 * X * 1024);  X0 = rint((M1 * Y + M2) * 1024) + 16;  Y0 = rint((M4 * Y + M5) * 1024) + 16
 *        Xq = (X0 + ad) >> 5;  Yq = (Y0 + bd) >> 5  (arithmetic);  sx = Xq >> 5;  sy = Yq >> 5;  fx = Xq & 31;  fy = Yq & 31
 *        taps p00 (sy, sx), p01 (sy, sx+1), p10 (sy+1, sx), p11 (sy+1, sx+1), every index mapped by BORDER_REFLECT_101 over the
 *        sample's own W_b / H_b (period 2(len-1), any number of reflections, len == 1 -> 0)
 *        images  v = (p00*(32-fy)*(32-fx) + p01*(32-fy)*fx + p10*fy*(32-fx) + p11*fy*fx + 512) >> 10;  x = (float)v / 255.f
 *        flow    gx = (float)fx / 32.f, gy alike;  w00 = (1-gy)*(1-gx), w01 = (1-gy)*gx, w10 = gy*(1-gx), w11 = gy*gx;
 *                f = ((p00*w00 + p01*w01) + p10*w10) + p11*w11 per plane;  u' = A00*fu + A01*fv;  v' = A10*fu + A11*fv
 *        valid   the 0/1 taps with the same weights and order (exact), valid = (sum > 0.5f) ? 1 : 0 (exactly 0.5 is NOT valid)
 *   flip: u' = u' * -1.0f last.
 * A record the kernel cannot honour -- h not in [1, Hs], w not in [1, Ws], crop_h > h, crop_w > w, or a crop origin outside
 * [0, h-crop_h] x [0, w-crop_w] -- never becomes a gather: that sample's outputs are zeros and status[b] = 1 (0 otherwise).  A matrix
 * with non-finite or huge entries is harmless: conversions saturate, sums wrap, and every tap index is reflected into the sample.
 * The reference's "upsize first when the frame is smaller than the crop" branch (:259-268) is not provided.
 * PWC_EINVAL, nothing launched: a null pointer (valid may be NULL), non-positive sizes, n > 65535, Hs or Ws > 32767 (OpenCV's short
 * coordinate saturation is not restated), crop_h > Hs or crop_w > Ws, gt_kind not 0 or 1, valid != NULL with gt_kind 1.
 * PWC_EALIGN, nothing launched: x / flow / valid_out / status / a float gt not 4-byte aligned, a uint16 gt not 2-byte aligned, params not
 * 8-byte aligned. */
typedef struct pwc_augment_params {
    double m[6];
    float a[4];
    int32_t y0, x0, h, w, warp, flip;
} pwc_augment_params;
int pwc_kitti_augment(const void *frames, const void *gt, int gt_kind, const void *valid /* may be NULL */, int n, int Hs, int Ws,
                      int crop_h, int crop_w, const void *params /* device pwc_augment_params [n] */, void *x, void *flow,
                      void *valid_out, void *status /* int32 [n] */, void *stream);

/* Training batches of train2.py on the device (addition within ABI v13, csrc/pwc_augment_full.hip): KittiAugmentationPipeline
 * (data_processing.py:136-279) -- random crop, horizontal flip, rotation up to +-17 degrees, integer translation, brightness /
 * contrast, Gaussian blur, /255 -- in one launch.  frames, gt, gt_kind, valid, the slot layout with the sample's own row stride, the
 * PNG decode and "valid == NULL -> all ones" are exactly those of pwc_kitti_augment above.  Outputs, all dense: x float
 * [n][6][crop_h][crop_w], flow float [n][2][crop_h][crop_w], mask_out float [n][1][crop_h][crop_w] -- FRACTIONAL after a rotation, the
 * reference does not threshold it again -- and status int32 [n].
 *
 * cv2 is DEFINED here by restatement, and parity against an actual cv2 build is UNPINNED in each of these points:
 *   cv2.warpAffine (INTER_LINEAR, BORDER_REFLECT) of float32 images: OpenCV's classic fixed-point coordinates (as above) and the
 *     float blend below;                                      parity against an actual cv2 build is unpinned
 *   cv2.getRotationMatrix2D(center, angle, 1.0) in float64;   parity against an actual cv2 build is unpinned
 *   cv2.GaussianBlur of 8U images: OpenCV's bit-exact fixed-point path (Q8.8 weights, uint16 horizontal pass, uint32 vertical pass,
 *     BORDER_REFLECT_101);                                    parity against an actual cv2 build is unpinned
 *   the Q8.8 weights are rounded from a FLOAT64 Gaussian, OpenCV computes it in softdouble: a stated, unpinned difference
 *   the flow rotation is float64 because cos / sin are NumPy float64 scalars, which promote the float32 planes UNDER NUMPY 2
 *     (checked on 2.2.6); under NumPy 1's value-based casting it would be float32: unpinned against other NumPy versions.
 * Everything is integer arithmetic, or fp32 / fp64 in the expression order below without fused multiply-add: the result is
 * bit-reproducible and bit-identical to tests/augment_full_oracle.py, which runs the stages in the reference's forward order.
 *
 * The reference crops FIRST: every later stage lives inside the crop_h x crop_w window, every border reflection is about the window's
 * edges, and frame pixels outside the window are never read.  Two foldings of an integer p into [0, len), any number of reflections:
 *   reflect(p, len)     BORDER_REFLECT      fedcba|abcdef|fedcba   m = p mod 2 len;      m < len ? m : 2 len - 1 - m
 *   reflect101(p, len)  BORDER_REFLECT_101  fedcb|abcdef|edcba     m = p mod 2 (len-1);  m < len ? m : 2 (len-1) - m;  len == 1 -> 0
 * One pwc_augment_full_params record (128 bytes, DEVICE buffer, 8-byte aligned) per sample:
 *   m[6]    the INVERTED rotation matrix in fp64: M = [[al, be, (1-al) cx - be cy], [-be, al, be cx + (1-al) cy]] with
 *           al = cos(angle pi/180), be = sin(angle pi/180), (cx, cy) = (crop_w / 2, crop_h / 2) in integer division, inverted as above
 *   cs[2]   cos and sin of the angle in fp64 (applied to the flow vectors)
 *   gain    (float)(brightness * contrast), the product taken in fp64
 *   wk[7]   the ksize Q8.8 weights of the blur in wk[0 .. ksize), summing to exactly 256;  ksize 3, 5 or 7
 *   y0, x0  crop origin;  h, w = H_b, W_b the sample's own size;  tx, ty the shift in pixels
 *   flip, rot, trans, bright, blur   stage flags (non-zero = on); the fields of a stage that is off are ignored
 * For output pixel (y, x) of the window the reference's stages are applied read-side, last stage first.  V(y, x) below is "the image
 * values, the flow vector and the mask after stages 6..2 at window position (y, x)":
 *   1 blur (images only):  s(j, i) = (uint8) trunc of the image value of V(reflect101(y + j, crop_h), reflect101(x + i, crop_w)),
 *        |i|, |j| <= (ksize-1)/2;  out = (sum_j sum_i w_j w_i s(j, i) + 32768) >> 16;  x = (float)out / 255.f
 *        (the horizontal sums fit uint16, the vertical uint32, nothing saturates because the weights add up to 256)
 *     no blur:  x = value / 255.f on the float value -- values are quantised only when the blur is on
 *   2 brightness / contrast (images only):  t = gain * (p - 127.5f) + 127.5f, each operation rounded to fp32;  p = min(max(t, 0), 255)
 *   3 translation:  (y, x) <- (reflect(y - ty, crop_h), reflect(x - tx, crop_w)), an exact gather (through the fixed-point warp an
 *        integer shift has fraction 0 and weights 1, 0, 0, 0)
 *   4 rotation:  ad, bd, X0, Y0, Xq, Yq, sx, sy, fx, fy as for pwc_kitti_augment, with (Y, X) = (y, x) in WINDOW coordinates;
 *        taps (ya, xa) = (reflect(sy, crop_h), reflect(sx, crop_w)), (yb, xb) = the same of sy + 1, sx + 1
 *        gx = (float)fx / 32.f, gy alike;  w00 = (1-gy)*(1-gx), w01 = (1-gy)*gx, w10 = gy*(1-gx), w11 = gy*gx
 *        every plane -- six image planes as (float)byte, u, v, mask:  f = ((p00*w00 + p01*w01) + p10*w10) + p11*w11
 *        then  u' = (float)((double)u * cs[0] - (double)v * cs[1]);  v' = (float)((double)u' * cs[1] + (double)v * cs[0])
 *        -- v' is computed from the ALREADY ROTATED u', as the reference does (its u is a view of the plane it has just overwritten)
 *   5 flip:  every window tap column xt becomes crop_w - 1 - xt, and u of every tap is negated before it is blended
 *   6 crop:  window tap (yt, xt) is pixel (y0 + yt, x0 + xt) of the sample
 * A record the kernel cannot honour -- h not in [1, Hs], w not in [1, Ws], crop_h > h, crop_w > w, a crop origin outside
 * [0, h-crop_h] x [0, w-crop_w], with blur on a ksize other than 3, 5, 7 or weights that do not add up to 256, with trans on |tx| or
 * |ty| > PWC_AUGMENT_FULL_MAX_SHIFT -- never becomes a gather: that sample's outputs are zeros and status[b] = 1 (0 otherwise).  Every
 * tap index is folded into the window whatever the matrix holds.  PWC_EINVAL / PWC_EALIGN, nothing launched: as pwc_kitti_augment. */
#define PWC_AUGMENT_FULL_MAX_SHIFT 32767
typedef struct pwc_augment_full_params {
    double m[6];
    double cs[2];
    float gain;
    uint16_t wk[7];
    uint16_t ksize;
    int32_t y0, x0, h, w, tx, ty;
    int32_t flip, rot, trans, bright, blur;
} pwc_augment_full_params;
int pwc_kitti_augment_full(const void *frames, const void *gt, int gt_kind, const void *valid /* may be NULL */, int n, int Hs, int Ws,
                           int crop_h, int crop_w, const void *params /* device pwc_augment_full_params [n] */, void *x, void *flow,
                           void *mask_out, void *status /* int32 [n] */, void *stream);

/* ---- fp16 convolution (first piece of the half-precision path, BASELINE configs 3-4) --------------------------
 * Activations are channel-blocked "c8": [B][ceil(C/8)][H][W][8] halves, channels past C zero; only the batch
 * stride (in halves, multiple of 8) is free, so a tensor may be a channel-group slice of an arena.  fp32
 * accumulation on v_mfma_f32_32x32x16_f16; bias fp32; optional LeakyReLU; output rounded to half with saturation
 * (|v| > 65504 -> +-65504, never inf), or left in fp32 with PWC_CONV_OUT_F32.
 * Same operator as pwc_conv2d_fwd (nn.Conv2d 3x3 + LeakyReLU, PWCNet.py:26-33): stride 1 with dilation 1,2,4,8,16 and
 * stride 2 with dilation 1 (PWC_EUNSUPPORTED otherwise; no residual flag). */
int64_t pwc_conv3x3_f16_packed_bytes(int Cin, int Cout);
/* w: [Cout,Cin,3,3] f32 (nn.Conv2d layout, device) -> wp: packed halves [Cg/2][tap][2][CoutP][8]. */
int pwc_conv3x3_f16_pack(const void *w, void *wp, int Cin, int Cout, void *stream);
/* Split filters: the same layout with CoutP = 32 * ceil(Cout / 16) -- every 32-row cout tile carries 16 filters rounded to half
 * (rows 0..15) and their rounding residuals times 2^11 (rows 16..31): y = sum(hi) + sum(lo)/2^11 in the epilogue of
 * pwc_conv2d_f16_fwd(PWC_CONV_SPLIT_W).  pwc_conv3x3_f16_packed_bytes_split bytes (= the plain size for Cout <= 16). */
int64_t pwc_conv3x3_f16_packed_bytes_split(int Cin, int Cout);
int pwc_conv3x3_f16_pack_split(const void *w, void *wp, int Cin, int Cout, void *stream);
int pwc_conv2d_f16_fwd(const void *x, const void *wp, const void *bias, void *y,
                       int B, int Cin, int H, int W, int Cout, int stride, int dilation,
                       unsigned flags, float leaky_slope, int64_t x_bstride, int64_t y_bstride, void *stream);
/* layout conversions at the edges of an fp16 pipeline: NCHW f32 <-> c8 f16 (batch strides in elements) */
int pwc_nchw_to_c8_f16(const void *x, void *y, int B, int C, int H, int W, int64_t x_bstride, int64_t y_bstride, void *stream);
/* the same keeping the rounding residual: y_hi = half(x), y_lo = half(x - y_hi), two c8 tensors of ceil(C/8) groups (strict
 * half-precision mode: a consumer whose filters are duplicated over both channel sets reads ~22-bit activations) */
int pwc_nchw_to_c8_f16_hilo(const void *x, void *y_hi, void *y_lo, int B, int C, int H, int W, int64_t x_bstride,
                            int64_t hi_bstride, int64_t lo_bstride, void *stream);
int pwc_c8_f16_to_nchw(const void *x, void *y, int B, int C, int H, int W, int64_t x_bstride, int64_t y_bstride, void *stream);

/* First pyramid layer (conv1a: Conv2d(3,16,3,stride 2,pad 1) + LeakyReLU, PWCNet.py:52) from a float32 NCHW image
 * x:[B,3,H,W] (batch stride free: a pair tensor [B,6,H,W] is two calls) straight to c8 halves y:[B,2,H/2,W/2,8];
 * w:[16,3,3,3] f32 (nn layout), bias:[16] f32. */
int pwc_image_conv_s2_c8_f16(const void *x, const void *w, const void *bias, void *y, int B, int H, int W,
                             float leaky_slope, int64_t x_bstride, int64_t y_bstride, void *stream);

/* conv1a -> conv1aa -> conv1b -> conv2a (PWCNet.py:52-55 as used at :184-187: the level-1 features feed conv2a only) in ONE
 * launch: x float32 [B,3,H,W] -> y c8 halves [B][4][H2][W2][8] with H1 = (H-1)/2+1, H2 = (H1-1)/2+1 (same for W).  The three
 * level-1 maps live in LDS per 8x16 output tile.  wpack: pwc_pyramid1_f16_packed_bytes() bytes of halves = conv1a as
 * [k/8][cout 16][k%8] (k = ci*9+ky*3+kx, 27 padded to 32), then conv1aa, conv1b ([20 rows = tap*2+kh, last two zero][16][8])
 * and conv2a ([20][32][8]); bias: float[80] = conv1a | conv1aa | conv1b | conv2a.  LeakyReLU(leaky_slope) after every layer. */
int64_t pwc_pyramid1_f16_packed_bytes(void);
int pwc_pyramid1_fused_f16(const void *x, const void *wpack, const void *bias, void *y, int B, int H, int W,
                           float leaky_slope, int64_t x_bstride, int64_t y_bstride, void *stream);

/* The 16 -> 16 layers of the fp32 first pyramid level (conv1aa, conv1b: Conv2d(16,16,3,pad 1) + LeakyReLU, PWCNet.py:53-54) by
 * Winograd F(2x2,3x3) on the fp32 matrix cores (csrc/pwc_pyr1_wino.hip): 16 multiplications per 2x2 outputs, the whole transformed
 * filter bank in LDS, no workspace.  x, y: float32 [B,16,H,W] with free batch strides (elements, multiples of 4), 16-byte aligned,
 * W % 4 == 0 (PWC_EUNSUPPORTED otherwise: such a layer stays on pwc_conv2d_fwd).  up = pwc_pyr1_wino_pack(w): G g Gt of w:[16,16,3,3]
 * in the order [16 positions][cin % 4][cout][cin / 4], pwc_pyr1_wino_packed_bytes() bytes.  The result differs from pwc_conv2d_fwd
 * by fp32 rounding only.
 * pwc_pyr1_wino_pair_fwd: two such layers (x -> up1, bias1 -> up2, bias2 -> y) in one launch; the map between them lives in LDS per
 * 14 x 60 output tile (its ring outside the image is zero: the second layer pads the first one's output).  x != y.
 * pwc_pyr1_wino_preferred: 0 = keep pwc_conv2d_fwd (option "pyr1_wino" = 0, W % 4 != 0, or fewer than "pyr1_wino_min_tiles" 8 x 64
 * tiles in the launch), 1 = layer by layer (the default), 2 = the pair in one launch (option "pyr1_wino" = 2; measured slower at
 * batch 16, kept for A/B runs). */
int64_t pwc_pyr1_wino_packed_bytes(void);
int pwc_pyr1_wino_preferred(int B, int H, int W);
int pwc_pyr1_wino_pack(const void *w, void *up, void *stream);
int pwc_pyr1_wino_fwd(const void *x, const void *up, const void *bias, void *y, int B, int H, int W, float leaky_slope,
                      int64_t x_bstride, int64_t y_bstride, void *stream);
int pwc_pyr1_wino_pair_fwd(const void *x, const void *up1, const void *bias1, const void *up2, const void *bias2, void *y,
                           int B, int H, int W, float leaky_slope, int64_t x_bstride, int64_t y_bstride, void *stream);

/* PWC-Net's cost volume (pad 4, kernel 1, max displacement 4, strides 1) on c8 f16 tensors, fp32 accumulation:
 * in1,in2: [B][ceil(C/8)][H][W][8]; out: [B][11][H][W][8] = 81 displacement channels ((dy+4)*9+(dx+4)) + 7 zeros.
 * flags: PWC_CORR_NORMALIZE (divide by C instead of multiplying by corr_multiply), PWC_ACT_LEAKY. */
int pwc_corr81_c8_f16(const void *in1, const void *in2, void *out, int B, int C, int H, int W,
                      float corr_multiply, unsigned flags, float leaky_slope,
                      int64_t in1_bstride, int64_t in2_bstride, int64_t out_bstride, void *stream);
/* PWCDCNet.warp on c8 f16 tensors.  flo: a c8 tensor whose channels flo_channel, flo_channel+1 (same group) hold
 * (u, v) -- e.g. the arena group that carries up_flow; coordinates and weights in fp32 as in pwc_warp_fwd. */
int pwc_warp_c8_f16(const void *x, const void *flo, void *out, int B, int C, int H, int W, int flo_channel,
                    float flow_scale, int align_corners, float mask_threshold,
                    int64_t x_bstride, int64_t flo_bstride, int64_t out_bstride, void *stream);
/* Entry of decoder level L < 6 on c8 f16 tensors in one pass (reference models/PWCNet.py:208-212, 222-226, 236-240,
 * 252-256: up_flow = deconv(flow), up_feat = upfeat(x), warp = self.warp(c2L, up_flow * s), then the concat).
 * The flow stays in fp32 from level to level:
 *   flow32: float [B][>=1][H/2][W/2][8] -- the level above's head convolution run with PWC_CONV_OUT_F32, flow (u,v) in
 *     channels 0,1;  deconv_w [2,2,4,4] / deconv_b [2] float: deconvL's nn.ConvTranspose2d parameters, applied here in
 *     fp32 (16 fma per output value);
 *   feat_phases: float [B][1][H/2][W/2][8] -- upfeatL computed as a 3x3 conv with 4 output phases per channel
 *     (pwc_conv2d_f16_fwd), channel index co*4 + py*2 + px;
 *   flow_group [B][1][H][W][8] halves: channels 0,1 <- up_flow, 2,3 <- up_feat (4..7 untouched) -- the arena's last group;
 *   c1_dst <- c1 (ceil(C/8) groups: the arena's c1 slot);  warped <- warp(c2, up_flow * flow_scale) with the fp32
 *     up_flow, taps and mask as pwc_warp_c8_f16.
 * H and W must be even.  Batch strides in elements of the tensor's own type. */
int pwc_level_entry_c8_f16(const void *c1, const void *c2, const void *flow32, const void *feat_phases,
                           const void *deconv_w, const void *deconv_b,
                           void *c1_dst, void *flow_group, void *warped, int B, int C, int H, int W,
                           float flow_scale, int align_corners, float mask_threshold,
                           int64_t c1_bstride, int64_t c2_bstride, int64_t flow32_bstride,
                           int64_t feat_phases_bstride, int64_t c1_dst_bstride, int64_t flow_group_bstride,
                           int64_t warped_bstride, void *stream);

/* pwc_level_entry_c8_f16 + pwc_corr81_c8_f16 in ONE launch, the warped features staying in LDS (PWCNet.py:208-214 for a level below
 * the coarsest): the flow group and the c1 slot of the arena are written as by pwc_level_entry_c8_f16, corr_out
 * [B][11][H][W][8] (81 channels + 7 zeros, LeakyReLU with PWC_ACT_LEAKY, PWC_CORR_NORMALIZE as in pwc_corr81_c8_f16) as by
 * pwc_corr81_c8_f16 on the warped tensor -- bit-identical to the two calls; no `warped` tensor is needed.  One launch less and no
 * round trip of the warped features through HBM, but every tile gathers its 16 x 40 halo (2.5x the pixels): 97 vs 81 us at level 2
 * of a batch of 16, faster only for single small launches; the plans keep the two calls unless option "f16_level_corr" is set. */
int pwc_level_corr81_c8_f16(const void *c1, const void *c2, const void *flow32, const void *feat_phases,
                            const void *deconv_w, const void *deconv_b,
                            void *c1_dst, void *flow_group, void *corr_out, int B, int C, int H, int W,
                            float flow_scale, int align_corners, float mask_threshold,
                            float corr_multiply, unsigned flags, float leaky_slope,
                            int64_t c1_bstride, int64_t c2_bstride, int64_t flow32_bstride,
                            int64_t feat_phases_bstride, int64_t c1_dst_bstride, int64_t flow_group_bstride,
                            int64_t corr_bstride, void *stream);

/* ConvTranspose2d(kernel 4, stride 2, padding 1) + bias.  x:[B,Cin,H,W], w:[Cin,Cout,4,4] (nn layout),
 * y:[B,Cout,2H,2W]. */
int pwc_deconv4x4s2_fwd(const void *x, const void *w, const void *bias, void *y,
                        int B, int Cin, int H, int W, int Cout, int dtype,
                        int64_t x_bstride, int64_t y_bstride,
                        void *stream);
/* Small levels (ABI v11): the host runs predict_flowL and upfeatL as ONE 3x3 convolution with 10 output channels -- ConvTranspose2d
 * (k4, s2, p1) is a 3x3 convolution with four output phases per channel -- through pwc_conv2d_fwd (matrix cores, split-K over the
 * chip) instead of pwc_deconv4x4s2_fwd, which is VALU-bound on the few CUs a small map gives it.  This is the level's exit:
 * head [B,10,h,w] = [flow u, v | upfeat phases co*4 + py*2 + px] -> out [B,4,2h,2w] = [deconvL(flow) | up_feat] (PWCNet.py:208-209,
 * 222-223, 236-237, 252-253); deconv_w [2,2,4,4], deconv_b [2] = deconvL's nn.ConvTranspose2d parameters.  Batch strides in elements. */
int pwc_upsample_entry_f32(const void *head, const void *deconv_w, const void *deconv_b, void *out, int B, int h, int w,
                           int64_t head_bstride, int64_t out_bstride, void *stream);

/* predict_flowL (Conv2d Cin->2, 3x3) and upfeatL (ConvTranspose2d Cin->2, k4 s2 p1) in ONE pass over x:
 * both read the same 3x3 window of the same [B,Cin,H,W] arena (PWCNet.py:207+209, 221+223, 235+237, 251+253).
 * head_wp = pwc_conv3x3_pack of the [2,Cin,3,3] head filters; up_w = [Cin,2,4,4] (nn layout).
 * flow:[B,2,H,W], up_out:[B,2,2H,2W].  Returns PWC_EUNSUPPORTED (nothing launched) when the geometry is
 * outside the streaming kernel (W % 4 != 0, W < 128, unaligned): call the two separate entry points then. */
int pwc_head_upfeat_fwd(const void *x, const void *head_wp, const void *head_bias, void *flow,
                        const void *up_w, const void *up_bias, void *up_out,
                        int B, int Cin, int H, int W, int dtype,
                        int64_t x_bstride, int64_t flow_bstride, int64_t up_bstride, void *stream);
/* The same with a scratch buffer of pwc_head_upfeat_workspace_bytes(B, Cin, H, W) bytes (0: this geometry never uses one; ABI v12):
 * launches of fewer than 256 8-row x 128-column tiles -- fewer workgroups than the chip has CUs, each VALU-bound on its own CU -- are
 * cut along Cin into slices (option "stream_slice_wgs") whose partial sums meet in the workspace and are added in fixed slice order:
 * deterministic; the fp32 summation order differs from the one-pass form.  workspace NULL / too small: the one-pass form.  With the
 * workspace the entry also takes launches of 4..63 tiles (PWC_EUNSUPPORTED without it, as pwc_head_upfeat_fwd). */
int64_t pwc_head_upfeat_workspace_bytes(int B, int Cin, int H, int W);
int pwc_head_upfeat_ws_fwd(const void *x, const void *head_wp, const void *head_bias, void *flow,
                           const void *up_w, const void *up_bias, void *up_out,
                           int B, int Cin, int H, int W, int dtype,
                           int64_t x_bstride, int64_t flow_bstride, int64_t up_bstride,
                           void *workspace, int64_t workspace_bytes, void *stream);

/* Adam / AdamW step with global-norm gradient clipping over all tensors of an optimizer (opticalflow_amd/optim.py): what the
 * reference's scripts do with clip_grad_norm_ + optimizer.step() (train2.py), Adam + L2 weight decay (train_pseudo.py,
 * train_fundamental.py) and GradScaler.step(optimizer) (train.py), as three launches -- square sum, finish, update -- without a host
 * synchronisation.  fp32 parameters, gradients and moments only.
 *
 * Every tensor is cut into chunks of pwc_optim_chunk_elems() elements, one workgroup each.  The caller keeps three device tables:
 *   tensors  [ntensors] {float *p, *m, *v; int64_t numel}    parameter, exp_avg, exp_avg_sq (dense); changes with the parameter set
 *   grads    [ntensors] const float *                        this step's gradients; NULL leaves the tensor out of the step
 *   chunks   [nchunks]  {int32 tensor, int32 chunk}          chunk `chunk` of tensor `tensor` = its elements [chunk * K, (chunk + 1) * K)
 * and a workspace of pwc_optim_workspace_bytes(nchunks, ngroups) bytes (8-byte aligned): one fp64 partial per chunk, then one record
 * of constants per parameter group.  The tables are trusted: an entry that does not describe live memory is a wild access.
 *
 * pwc_optim_grad_sqsum   partial[i] = sum of g^2 over chunk i, each product and the sum in fp64, fixed order, no atomics.
 * pwc_optim_finish       for one group: the partials added in index order, total_norm = (float)sqrt(sum) * (1 / grad_scale),
 *                        coef = min(1, max_norm / (total_norm + 1e-6f)) in fp32 (torch's clip_grad_norm_); clip = 0: partials not
 *                        read, coef = 1, norm_out not written.  found_inf / grad_scale: optional fp32 device scalars (GradScaler's
 *                        protocol for optimizers with _step_supports_amp_scaling).  found_inf != 0 marks the step skipped;
 *                        otherwise step_record[group] = {double step, beta1^step, beta2^step} advances by one step (running
 *                        products).  The group's constants {step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step),
 *                        each formed in fp64 and rounded once, coef, 1 / grad_scale, skipped} go to the workspace and total_norm to
 *                        norm_out.  A new record is {0, 1, 1}.
 * pwc_optim_adam_update  chunks [chunk_begin, chunk_begin + chunk_count) (one group's) with the group's constants; per element,
 *                        in fp32 and in this order (nothing is written when the step is skipped; g itself is never modified):
 *                          g = (g * inv_scale) * coef;  weight_decay != 0: g = g + wd * p (L2) or p = p * (1 - lr * wd) (decoupled)
 *                          m = m + (1 - b1) * (g - m);  v = v * b2 + (1 - b2) * (g * g)
 *                          p = p + (-step_size) * (m / (sqrt(v) / bc2_sqrt + eps))
 *                        with correctly rounded division and square root, and 1 - b1, 1 - b2, 1 - lr * wd formed in fp64 and rounded
 *                        once.  16-byte accesses where g, p, m and v of a tensor are all 16-byte aligned, 4-byte ones otherwise. */
int pwc_optim_chunk_elems(void);
int64_t pwc_optim_workspace_bytes(int64_t nchunks, int ngroups);
int pwc_optim_grad_sqsum(const void *grads, const void *tensors, const void *chunks, int64_t nchunks, int ngroups,
                         void *workspace, int64_t workspace_bytes, void *stream);
int pwc_optim_finish(void *workspace, int64_t workspace_bytes, int64_t nchunks, int ngroups, int group, int clip,
                     double max_norm, const void *found_inf, const void *grad_scale, double lr, double beta1,
                     double beta2, void *step_record, void *norm_out, void *stream);
int pwc_optim_adam_update(const void *grads, const void *tensors, const void *chunks, int64_t nchunks, int64_t chunk_begin,
                          int64_t chunk_count, int ngroups, int group, const void *workspace, int64_t workspace_bytes,
                          double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                          void *stream);

/* Profiling calibration, not on the product path: streams `nbytes` (a multiple of 64*width) of src through LDS with the
 * kernels' own LDS-DMA instruction (width 4: buffer_load_dword ... lds, width 16: buffer_load_dwordx4 ... lds) so that rocprofv3's
 * FETCH_SIZE can be calibrated on a known byte count in this access pattern (MI355X guide, HBM section).  sums: blocks*256 floats. */
int pwc_calib_lds_dma_read(const void *src, void *sums, int64_t nbytes, int width, int blocks, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PWC_HIP_H_ */
