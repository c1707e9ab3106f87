/* gz_ops.h -- C ABI of libgz_hip.so: the MI355X (gfx950) kernels behind the G+D training step of
 * ebartrum/lightning_gan_zoo.
 *
 * The reference has no FFI of its own: its hot path is torch.nn operator calls made from
 *   core/models/standard_networks.py:9-93        (DCGAN/WGAN generator + discriminator)
 *   core/lightning_module.py:104-128,158-207     (DCGAN / WGAN / WGANGP training_step)
 *   core/utils/utils.py:39-58                    (gradient_penalty)
 * Each entry point below replaces the aten operator(s) named in its comment; the Python side
 * (lightning_gan_zoo_amd/functional/) binds them with ctypes and wraps them in
 * torch.autograd.Function objects (see INTEGRATION.md for the binding a maintainer would add).
 *
 * Conventions
 *   - plain pointers to DEVICE memory, fp32, contiguous NCHW; sizes as int; no torch types.
 *   - every launcher takes the HIP stream explicitly, never synchronises, never allocates, and is
 *     re-entrant (autograd runs backward on its own thread).
 *   - return value: 0 on success, negative error code otherwise (GZ_ERR_*); never throws.
 *   - workspaces are caller-allocated; *_workspace_bytes / *_elems tell how much.
 */
#ifndef GZ_OPS_H
#define GZ_OPS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define GZ_ACT_NONE 0
#define GZ_ACT_RELU 1
#define GZ_ACT_LRELU 2
#define GZ_ACT_TANH 3

/* ---- convolution family -------------------------------------------------------------------
 * Geometry names: x [N,C,H,W] is the image side, y [N,K,OH,OW] the feature side,
 * w [K,C,KH,KW] the Conv2d weight (a ConvTranspose2d weight [Cin,Cout,KH,KW] is the same array
 * with K = Cin, C = Cout).  Supported (KH,KW,S,P): (4,4,2,1) (5,5,2,2) (3,3,1,1) (1,1,1,0).
 */

/* packed-weight sizes in floats */
long long gz_conv2d_pack_fwd_elems(int K, int C, int KH, int KW);
long long gz_conv2d_pack_dgrad_elems(int K, int C, int KH, int KW, int S);

/* w -> [C*KH*KW][round4(K)] GEMM-B image for gz_conv2d_fwd */
int gz_conv2d_pack_fwd(const float* w, float* wpack, int K, int C, int KH, int KW, hipStream_t stream);
/* w -> [S*S phases][K*TY*TX][round4(C)] GEMM-B images for gz_conv2d_dgrad */
int gz_conv2d_pack_dgrad(const float* w, float* wpack, int K, int C, int KH, int KW, int S, int P,
                         hipStream_t stream);
/* Re-packing every weight of a network in ONE launch (the packs follow each optimizer step: ~15 launches per G+D pair).
 * gz_conv2d_pack_job fills one host-side job record (gz_conv2d_pack_job_bytes() bytes) for the pair (w, wp) -- the
 * same image gz_conv2d_pack_fwd / _dgrad would write -- and returns the number of workgroups it needs (its first one is
 * `block0` = the sum over the jobs before it); the records are copied to the device as one array and
 * gz_conv2d_pack_multi runs them all. */
size_t gz_conv2d_pack_job_bytes(void);
int gz_conv2d_pack_job(void* job_out, const float* w, float* wp, int is_dgrad, int K, int C, int KH, int KW, int S, int P,
                       int block0);
int gz_conv2d_pack_multi(const void* jobs_dev, int njobs, int total_blocks, hipStream_t stream);
/* Packed images with the job table passed by value and an optional scale 1 / sigma[0] (sigma on the device, may be
 * NULL): spectral normalisation's w = weight_orig / sigma is a new tensor at every call; one launch writes w (what = 2:
 * plain scaled copy) and the forward (what = 0) and dgrad (what = 1) images of every such layer.  table_host:
 * gz_conv2d_pack_table_bytes() zeroed host bytes, at most gz_conv2d_pack_table_max_jobs() jobs. */
int gz_conv2d_pack_table_max_jobs(void);
size_t gz_conv2d_pack_table_bytes(void);
int gz_conv2d_pack_table_add(void* table_host, const float* w, float* wp, const float* sigma, int what, int K, int C, int KH,
                             int KW, int S, int P);
int gz_conv2d_pack_table_launch(void* table_host, hipStream_t stream);

/* y = act(conv2d(x, w) + bias).  Replaces aten::convolution for nn.Conv2d forward
 * (standard_networks.py:20-24,36-43) and the input gradient of nn.ConvTranspose2d. */
int gz_conv2d_fwd(const float* x, const float* wpack, const float* bias, float* y, float* workspace, size_t ws_bytes,
                  int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P, int act,
                  float slope, hipStream_t stream);
/* Split-K scratch of gz_conv2d_fwd / gz_conv2d_dgrad / gz_gemm: launches whose output has too few tiles to fill
 * the 256 CUs (deep 4x4 / 8x8 maps at small batch, nn.Linear heads with K = 8192) cut the reduction instead and
 * sum the partial tiles in a second pass.  0 = not split.  A NULL / too small workspace is not an error: the
 * launch then runs unsplit. */
size_t gz_conv2d_fwd_workspace_bytes(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P);
size_t gz_conv2d_dgrad_workspace_bytes(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S,
                                       int P);
size_t gz_gemm_workspace_bytes(int M, int N, int K);

/* x = act(conv_transpose2d(y, w) + bias).  Replaces nn.ConvTranspose2d forward
 * (standard_networks.py:60-73,80-87) and aten::convolution_backward's grad_input for nn.Conv2d. */
int gz_conv2d_dgrad(const float* y, const float* wpack, const float* bias, float* x, float* workspace,
                    size_t ws_bytes, int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P,
                    int act, float slope, hipStream_t stream);

/* dw[K,C,KH,KW] = weight gradient.  Replaces aten::convolution_backward's grad_weight. */
size_t gz_conv2d_wgrad_workspace_bytes(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW);
/* dbias[K] (may be NULL) = sum over pixels of y, the bias gradient: produced in the same pass only by the
 * launches gz_conv2d_wgrad_fuses_bias reports (3x3 s1 p1 with few channels); otherwise pass NULL and reduce y */
int gz_conv2d_wgrad_fuses_bias(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P);
int gz_conv2d_wgrad(const float* x, const float* y, float* dw, float* dbias, float* workspace, size_t ws_bytes, int N,
                    int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P, hipStream_t stream);

/* Round 4 -- CU budget.  The convolution plans size their tile / split choices to whole rounds of workgroup slots on
 * `cu_count` CUs (default 256 = the whole MI355X).  Under data parallelism RCCL's channel kernels occupy part of the
 * chip while backward runs (the overlap ddp.GradSync creates); a plan sized for 256 CUs then spills into a second,
 * nearly empty round.  ddp.GradSync calls gz_set_cu_budget(256 - reserved) when world > 1 (clamped to [64, 256];
 * <= 0 restores 256); returns the value in effect.  Process-wide, may be changed between launches; workspace sizes and
 * gz_conv2d_plan follow it. */
int gz_set_cu_budget(int cu_count);
int gz_get_cu_budget(void);

/* Round 4 -- the dispatch as data.  gz_conv2d_plan writes a one-line description of the kernel a launch of op (0 F, 1 Dg,
 * 2 Wg) with this shape takes -- skeleton (igemm / igemm2 / igemm2w / a direct kernel), tile, operand loaders, number of
 * reduction slabs, BatchNorm statistics rows -- into buf; returns the text length or a negative error.  Pure host logic
 * (callable without a GPU); tests/test_dispatch_plan.py pins it for every layer of the BASELINE configurations, so a
 * heuristic edit that moves a layer onto another kernel shows up as a diff.  Describes the launch for 16-byte aligned
 * tensors with the advertised workspace. */
int gz_conv2d_plan(int op, int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P, char* buf,
                   int buflen);

/* Round 4 -- weight gradients straight into the optimizer's (or the gradient exchange's) buffer.
 * gz_conv2d_wgrad_partial: as gz_conv2d_wgrad, but a launch that splits its reduction leaves the slabs in `workspace`
 * and reports them (*nz_out slabs, *stride_out floats apart); *nz_out == 1 means dw is complete.  gz_reduce_multi then
 * sums the slabs of many parameters -- and of several launches per parameter (a discriminator applied to a real and a
 * fake batch) -- in ONE launch, writing (beta 0) or accumulating into (beta 1) each gradient.  Replaces the per-layer
 * slab reductions plus autograd's `grad += new` launches (reference: torch's AccumulateGrad behind every Conv2d /
 * ConvTranspose2d weight of core/models/standard_networks.py:20-24,36-43,60-73).  The table is plain host memory of
 * gz_reduce_multi_table_bytes() bytes, zero-initialised, filled with gz_reduce_multi_add (at most
 * gz_reduce_multi_max_jobs() gradients of gz_reduce_multi_max_sources() launches each; counts and strides multiples
 * of 4 floats, 16-byte aligned pointers). */
int gz_conv2d_wgrad_partial(const float* x, const float* y, float* dw, float* workspace, size_t ws_bytes, int N, int C,
                            int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P, int* nz_out,
                            long long* stride_out, hipStream_t stream);
/* Round 5 -- the first-order backward of `act(conv(x) + bias)` for the critics' first layer (k4 s2 p1, <= 4 image
 * channels, act = ReLU / LeakyReLU; reference core/models/standard_networks.py:62-66: Conv2d(3, features_d, 4, 2, 1) +
 * LeakyReLU(0.2)) in ONE launch: gy is the gradient with respect to the activation's OUTPUT, masked on load with the
 * saved forward output fwd_out; every slab row holds the K * C * 16 weight-gradient partial sums followed, at
 * *bias_offset_out, by the K bias-gradient partial sums.  Always partial: sum the *nz_out rows (*stride_out floats
 * apart) with gz_reduce_multi or hand them to gz_adam_step_from_slabs.  workspace: gz_conv2d_wgrad_workspace_bytes.
 * gz_conv2d_wgrad_act_fuses reports whether the shape takes this path (otherwise: gz_act_bwd + gz_conv2d_wgrad). */
int gz_conv2d_wgrad_act_fuses(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P, int act);
int gz_conv2d_wgrad_act_partial(const float* x, const float* gy, const float* fwd_out, int act, float slope,
                                float* workspace, size_t ws_bytes, int N, int C, int H, int W, int K, int OH, int OW,
                                int KH, int KW, int S, int P, int* nz_out, long long* stride_out,
                                long long* bias_offset_out, hipStream_t stream);
/* ... and the same layer's INPUT gradient (the generator step through the frozen critic): x = conv_transpose(gy *
 * act'(fwd_out), w) by the direct few-channel kernel with the mask formed on load.  gz_conv2d_dgrad_act_fuses reports
 * whether the shape takes it (otherwise: gz_act_bwd + gz_conv2d_dgrad); 16-byte aligned tensors, the dgrad weight pack. */
int gz_conv2d_dgrad_act_fuses(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P, int act);
int gz_conv2d_dgrad_act(const float* gy, const float* fwd_out, int act, float slope, const float* wpack, float* x, int N,
                        int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P, hipStream_t stream);
int gz_reduce_multi_max_jobs(void);
int gz_reduce_multi_max_sources(void);
size_t gz_reduce_multi_table_bytes(void);
int gz_reduce_multi_add(void* table_host, float* out, long long count, int beta, const float* slabs, int nz,
                        long long stride);
int gz_reduce_multi(void* table_host, hipStream_t stream);

/* Convolution + BatchNorm statistics in one launch (standard_networks.py:34-44,80-88: conv / transpose_conv ->
 * batch_norm): the epilogue also writes, per output channel and per group of pixels, (sum, sum of squares) of the
 * raw convolution output to stats[rows][channels][2]; gz_batchnorm_finalize turns them into the coefficients and
 * the running buffers -- the separate read of the whole feature map goes away.  *_stats_rows = number of partial
 * rows the launch produces, 0 when it cannot fuse (split-K launch, 3-channel direct kernel): use the plain entry
 * point + gz_batchnorm_stats then.  No bias, no activation (the activation follows the normalisation). */
int gz_conv2d_fwd_stats_rows(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P);
int gz_conv2d_fwd_stats(const float* x, const float* wpack, float* y, float* stats, int N, int C, int H, int W, int K,
                        int OH, int OW, int KH, int KW, int S, int P, hipStream_t stream);
int gz_conv2d_dgrad_stats_rows(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P);
/* Round 4: launches that split their reduction carry the statistics too -- the finish pass runs the same epilogue per
 * 32 x 32 output block (one partial row per 32 pixels) -- and need the op's workspace (gz_conv2d_{fwd,dgrad}_workspace_bytes).
 * The entry points without a workspace remain for unsplit plans. */
int gz_conv2d_fwd_stats_ws(const float* x, const float* wpack, float* y, float* stats, float* workspace, size_t ws_bytes,
                           int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P,
                           hipStream_t stream);
int gz_conv2d_dgrad_stats_ws(const float* y, const float* wpack, float* x, float* stats, float* workspace,
                             size_t ws_bytes, int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S,
                             int P, hipStream_t stream);
int gz_conv2d_dgrad_stats(const float* y, const float* wpack, float* x, float* stats, int N, int C, int H, int W, int K,
                          int OH, int OW, int KH, int KW, int S, int P, hipStream_t stream);

/* diagnostic: tile configuration a launch would use (op 0 F, 1 Dg, 2 Wg) -> 0 128x128, 1 128x64, 2 128x32, 3 64x64 */
int gz_conv2d_tile(int op, int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S);

/* c[M,N] = act(op(a) . op(b) + bias[n]); trans_a: a stored [K][M]; trans_b: b stored [N][K].
 * Replaces the 1x1 -> 4x4 ConvTranspose2d of the generator's first block (standard_networks.py:60),
 * its weight gradient, and nn.Linear. */
int gz_gemm(const float* a, const float* b, const float* bias, float* c, float* workspace, size_t ws_bytes, int M,
            int N, int K, int lda, int ldb, int ldc, int trans_a, int trans_b, int act, float slope,
            hipStream_t stream);

/* ---- cubic 3-D convolution family (HoloGAN ConvTranspose3d k3 s2 p1 op1, hologan_generator.py:29-30) ------
 * x [N,C,D,H,W] image side, y [N,K,OD,OH,OW] feature side, w [K,C,KS,KS,KS]; only (KS,S,P) = (3,2,1). */
long long gz_conv3d_pack_fwd_elems(int K, int C, int KS);
long long gz_conv3d_pack_dgrad_elems(int K, int C, int KS, int S);
int gz_conv3d_pack_fwd(const float* w, float* wpack, int K, int C, int KS, hipStream_t stream);
int gz_conv3d_pack_dgrad(const float* w, float* wpack, int K, int C, int KS, int S, int P, hipStream_t stream);
/* Each launcher decides its kernel once (skeleton, tile, reduction splits) from the shape and from what the call brings;
 * the *_workspace_bytes of an op is what the slabs of that decision need, 0 when it does not split.  A workspace that
 * is NULL or smaller than that:
 *   gz_conv3d_fwd / _dgrad planned on the igemm2 skeleton   return GZ_ERR_WORKSPACE and launch nothing;
 *   gz_conv3d_fwd / _dgrad planned on igemm                 run unsplit (same result up to summation order);
 *   gz_conv3d_wgrad                                         uses floor(ws_bytes / (4 * K * C * KS^3)) splits, unsplit
 *                                                           below 2 (same result up to summation order).
 * gz_conv3d_plan says which of these a shape is. */
/* y = act(conv3d(x, w) + bias): input gradient of nn.ConvTranspose3d.  wpack and y 16-byte aligned. */
int gz_conv3d_fwd(const float* x, const float* wpack, const float* bias, float* y, float* workspace, size_t ws_bytes,
                  int N, int C, int D, int H, int W, int K, int OD, int OH, int OW, int KS, int S, int P, int act,
                  float slope, hipStream_t stream);
size_t gz_conv3d_fwd_workspace_bytes(int N, int C, int K, int OD, int OH, int OW, int KS);
size_t gz_conv3d_dgrad_workspace_bytes(int N, int C, int K, int OD, int OH, int OW, int KS);
/* x = act(conv_transpose3d(y, w) + bias): nn.ConvTranspose3d forward.  wpack 16-byte aligned; D, H, W even. */
int gz_conv3d_dgrad(const float* y, const float* wpack, const float* bias, float* x, float* workspace,
                    size_t ws_bytes, int N, int C, int D, int H, int W, int K, int OD, int OH, int OW, int KS, int S,
                    int P, int act, float slope, hipStream_t stream);
size_t gz_conv3d_wgrad_workspace_bytes(int N, int C, int K, int OD, int OH, int OW, int KS);
int gz_conv3d_wgrad(const float* x, const float* y, float* dw, float* workspace, size_t ws_bytes, int N, int C, int D,
                    int H, int W, int K, int OD, int OH, int OW, int KS, int S, int P, hipStream_t stream);
/* the launch of op (0 F, 1 Dg, 2 Wg) as text, conventions of gz_conv2d_plan (host only; 16-byte aligned tensors and the
 * advertised workspace assumed): "<op> <skeleton><<tile>> <loader> splits=<n> slabs=<n>"; splits cut the reduction (of
 * the longest of Dg's 8 phases), slabs are the workspace slices that gives (summed over Dg's phases) */
int gz_conv3d_plan(int op, int N, int C, int D, int H, int W, int K, int OD, int OH, int OW, int KS, int S, int P,
                   char* buf, int buflen);

/* ---- HoloGAN rigid-body resampling (hologan_generator.py:198-321 + the permute/flip/reshape of :130-133) ----
 * vox [N,C,S,S,S]; minv [N,16] row-major inverse transforms; out2d [N, C*S, S, S] with
 * out2d[n][c*S + (S-1-y)][z][x] = trilinear(vox[n][c], minv[n] . (x,y,z,1)).  idx_out (may be NULL):
 * int64 [8][N*S^3], the clamped corner indices in the reference's idx_a..idx_h order. */
int gz_rigid_resample_fwd(const float* vox, const float* minv, float* out2d, long long* idx_out, int N, int C, int S,
                          hipStream_t stream);
/* gvox [N,C,S,S,S] = adjoint of the above in gather form (no atomics, every element written once): per-voxel hit
 * lists in `workspace` (gz_rigid_resample_bwd_workspace_bytes), gradient volumes staged through LDS.  workspace
 * NULL / too small: the same result from the slower direct gather.
 * A list holds at most gz_rigid_resample_bwd_list_capacity() hits; one source voxel with more (views that zoom in)
 * makes the whole launch take the direct gather.  Which of the two ran is decided on the device; after a call that was
 * given a sufficient workspace (16-byte aligned, as gout2d; S^3 % 4 == 0, S <= 16) it can be read back from the
 * workspace, in stream order, with capacity = gz_rigid_resample_bwd_list_capacity():
 *   - the int32 at byte offset gz_rigid_resample_bwd_workspace_bytes(N, S) - 16 is non-zero exactly when a list
 *     overflowed and the direct gather produced gvox;
 *   - the int32 plane [N*S^3] at byte offset capacity * N*S^3 * 4 holds min(hits, capacity) per source voxel
 *     (index n*S^3 + (z*S + y)*S + x). */
int gz_rigid_resample_bwd_list_capacity(void);
size_t gz_rigid_resample_bwd_workspace_bytes(int N, int S);
int gz_rigid_resample_bwd(const float* gout2d, const float* minv, float* gvox, float* workspace, size_t ws_bytes,
                          int N, int C, int S, hipStream_t stream);

/* gz_rigid_resample_fwd under V views of each of B sources (figures' view sweeps, forward only): vox [B,C,S,S,S],
 * minv [B*V,16] (row b*V+v), out2d [B*V, C*S, S, S] in gz_rigid_resample_fwd's layout, bit-equal to it applied to
 * the sources repeated V times; each source is read from HBM once per view chunk instead of once per view.
 * Needs S^3 % 4 == 0, a 16-byte aligned vox and 4*S^3 floats of LDS (S <= 16). */
int gz_rigid_resample_views_fwd(const float* vox, const float* minv, float* out2d, int B, int V, int C, int S,
                                hipStream_t stream);

/* ---- figures (core/figures/types.py): F frames of n images img [F*n, C, H, W] (C = 1 or 3) laid out as
 * torchvision's make_grid (ncol per row, padding / pad_value, one image unpadded), clamped to [0, 1], x * 255.0f in
 * fp32 truncated: out uint8 [F, GH, GW, 3] (4-byte aligned); GH x GW = make_grid's size for n images. */
int gz_figure_frames_u8(const float* img, unsigned char* out, int F, int n, int C, int H, int W, int ncol, int padding,
                        float pad_value, hipStream_t stream);

/* ---- evaluation path: InceptionV3 feature extractor of FID / KID (core/callback_inception_metrics.py:183-246,
 * core/submodules/gan_stability/metrics/inception.py) -- forward only --------------------------------------------
 * y = act(conv2d(x, w) + bias) for ANY rectangular kernel, per-axis stride and padding (3x3 s2 p0, 5x5 s1 p2,
 * 1x7 / 7x1, 1x3 / 3x1 ...).  Eval-mode BatchNorm is folded into w and bias by the caller.  wpack from
 * gz_conv2d_pack_fwd_any (tap-major, channels padded to 16). */
long long gz_conv2d_pack_fwd_any_elems(int K, int C, int KH, int KW);
int gz_conv2d_pack_fwd_any(const float* w, float* wpack, int K, int C, int KH, int KW, hipStream_t stream);
size_t gz_conv2d_fwd_any_workspace_bytes(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int SH,
                                         int SW, int PH, int PW);
int gz_conv2d_fwd_any(const float* x, const float* wpack, const float* bias, float* y, float* workspace,
                      size_t ws_bytes, int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int SH, int SW,
                      int PH, int PW, int act, float slope, hipStream_t stream);
/* The same convolution written into a channel slice of a concatenated tensor (InceptionV3's torch.cat of branch
 * outputs, inception.py:92-94 etc.): y points at the slice's first channel inside image 0, images are
 * y_image_channels * OH * OW floats apart.  Only the LDS-DMA launch takes a destination stride: GZ_ERR_UNSUPPORTED (-2)
 * when the shape runs elsewhere -- the caller then convolves into a temporary and copies. */
int gz_conv2d_fwd_any_into(const float* x, const float* wpack, const float* bias, float* y, int y_image_channels, int N,
                           int C, int H, int W, int K, int OH, int OW, int KH, int KW, int SH, int SW, int PH, int PW,
                           int act, float slope, hipStream_t stream);
/* square-window pooling over `planes` = N*C images; mode 0 max, 1 average with count_include_pad=False (the FID
 * network's patched pools), 2 average over KS*KS.  nn.AdaptiveAvgPool2d(1) = KS = H, S = 1, P = 0, mode 2. */
int gz_pool2d(const float* x, float* y, long long planes, int H, int W, int OH, int OW, int KS, int S, int P, int mode,
              hipStream_t stream);
/* The launch gz_pool2d makes for these arguments, as one line of text: "global_avg<16> grid=..", "band<3,2> grid=..
 * lds=..", "group<3,1,1> G=.. grid=.. lds=..", "group<3,2,0> ..", "plane grid=.. lds=..", "flat grid=..".  Host only (no
 * HIP call, no GPU needed); launcher and text read one choice.  x_aligned16: whether x is 16-byte aligned.  knobs: -1
 * the switches of this process, otherwise bit 0 = GZ_NO_POOL_GROUP, bit 1 = GZ_NO_POOL_PLANE.  Returns the length. */
int gz_pool2d_plan(long long planes, int H, int W, int OH, int OW, int KS, int S, int P, int mode, int x_aligned16,
                   int knobs, char* buf, int buflen);
/* y = F.interpolate(x, (OH, OW), mode='bilinear', align_corners=False) * mul + add */
int gz_resize_bilinear(const float* x, float* y, long long planes, int H, int W, int OH, int OW, float mul, float add,
                       hipStream_t stream);
/* Generator output -> InceptionV3 input in one launch (the device evaluation pass, eval.SampleDump.device_batches):
 * x [N, C, H, W] with C = 1 or 3, y [N, 3, OH, OW] = bilinear(q(x)) * mul + add, q(v) = ToTensor of the grey level
 * trunc(clamp(v, 0, 1) * 255) -- the callback's clamp -> (samples * 255).astype(int) -> PNG -> ToTensor, in fp32.  For
 * C = 1 the single plane feeds all three output channels.  Bit-equal to quantising on the host, then gz_u8hwc_to_nchw
 * (mean 0, std 1), then gz_resize_bilinear(..., mul, add): the three share their expressions.  GZ_ERR_BAD_SHAPE: a size
 * below 1, another C, a null pointer. */
int gz_samples_to_inception_input(const float* x, float* y, int N, int C, int H, int W, int OH, int OW, float mul,
                                  float add, hipStream_t stream);

/* ---- loss heads and the scalar side of spectral normalisation (csrc/gz_loss.hip) -----------------------------
 * Scalars (loss, sigma, the incoming loss gradient) are 1-element DEVICE arrays: nothing synchronises with the host.
 * loss[0] = mean_i BCE-with-logits(x[i], target), target a constant 0 or 1: criterion(logits, ones_like(logits)) /
 * zeros_like of core/lightning_module.py:114-119,126,221-235 */
int gz_bce_logits_mean(const float* x, float* loss, int n, float target, hipStream_t stream);
/* dx[i] = (sigmoid(x[i]) - target) * gloss[0] / n */
int gz_bce_logits_mean_bwd(const float* x, const float* gloss, float* dx, int n, float target, hipStream_t stream);
/* Round 4: the loss head of a discriminator step on the stacked batch [real; fake] (2 * n_each logits) in one launch.
 * mode 0: (mean BCE(x[:n], t0) + mean BCE(x[n:], t1)) / 2 (core/lightning_module.py:114-120);
 * mode 1: t0 * mean(x[:n]) + t1 * mean(x[n:]) (the WGAN critic loss with t0 = -1, t1 = +1, :168). */
int gz_pair_loss(const float* x, float* loss, int n_each, float t0, float t1, int mode, hipStream_t stream);
int gz_pair_loss_bwd(const float* x, const float* gloss, float* dx, int n_each, float t0, float t1, int mode,
                     hipStream_t stream);
/* loss[0] = mean((a - b)^2): HoloGAN's q_loss (:226,234);  da[i] = 2 (a[i] - b[i]) gloss[0] / n */
/* WGAN-GP penalty tail, core/utils/utils.py:55-57: out[0] = mean_n (sqrt(sumsq[n]) - 1)^2 and its gradient
 * dsumsq[n] = gout[0] (sqrt(s) - 1) / (sqrt(s) N), 0 where s == 0 (torch.norm's subgradient at the origin) */
int gz_gp_penalty(const float* sumsq, float* out, int n, hipStream_t stream);
int gz_gp_penalty_bwd(const float* sumsq, const float* gout, float* dsumsq, int n, hipStream_t stream);
int gz_mse_mean(const float* a, const float* b, float* loss, int n, hipStream_t stream);
int gz_mse_mean_bwd(const float* a, const float* b, const float* gloss, float* da, int n, hipStream_t stream);
/* torch.nn.utils.spectral_norm (core/models/hologan_discriminator.py:15): out = x / max(||x||, eps) (in place
 * allowed; the same values also to out2; out, out2, norm_out may be NULL), norm_out[0] = ||x||; out[0] = <a, b>; out = x / sigma[0]; and the gradient of
 * w = W / sigma(W), sigma = u^T W v:  out[r][l] = (g[r][l] - (sum_r rowdots[r]) u[r] v[l]) / sigma[0] with
 * rowdots[r] = <g[r], w[r]> (gz_rowdot). */
int gz_vec_normalize(const float* x, float* out, float* out2, float* norm_out, int n, float eps, hipStream_t stream);
/* gz_vec_normalize that also returns dot_out[0] = <x / max(||x||, eps), x>: with x = W v this is the power iteration's
 * u update and sigma = u^T W v in one launch */
int gz_vec_normalize_dot(const float* x, float* out, float* out2, float* dot_out, int n, float eps,
                         hipStream_t stream);
int gz_vec_dot(const float* a, const float* b, float* out, int n, hipStream_t stream);
/* The power iteration of SEVERAL spectral-normalised weights in four launches (every spectral-norm layer of one
 * discriminator call, core/models/hologan_discriminator.py:15,32): per job v <- normalise(W^T u), u <- normalise(W v),
 * sigma = u^T W v; u, v are the module's buffers (updated in place), us / vs / sigma the copies the autograd node keeps.
 * table_host: gz_sn_table_bytes() zeroed host bytes filled by gz_sn_add (at most gz_sn_max_jobs()); workspace:
 * gz_sn_workspace_floats(R, L) floats per job.  L % 4 == 0; W, v, vs, workspace 16-byte aligned. */
int gz_sn_max_jobs(void);
size_t gz_sn_table_bytes(void);
long long gz_sn_workspace_floats(int R, int L);
int gz_sn_add(void* table_host, const float* W, float* u, float* v, float* us, float* vs, float* sigma, float* workspace,
              int R, int L);
int gz_sn_power_iteration(void* table_host, float eps, hipStream_t stream);
/* A spectral-normalised convolution followed by InstanceNorm (no affine) without the per-call weight copy
 * (core/models/hologan_discriminator.py:28-38): IN_eps(conv(x, W / sigma) + b) = IN_{eps sigma^2}(conv(x, W)), so the
 * convolution runs on weight_orig's own packed images and the InstanceNorm takes one eps per sample.
 *   gz_rownorm_act_fwd_sigma (below): the InstanceNorm + activation with eps * sigma[g]^2 for the samples of group g
 *     (groups: discriminator calls stacked along n, sigma[groups] on the device)
 *   gz_sn_sigma_term: the gradient's sigma term, term[R][L] = sum_g coefs[g] u[g] v[g]^T with coefs[g] = dL/dsigma_g =
 *     -eps sigma_g sum_{rows of g} rstd^2 S2 from the backward's row sums (gz_rownorm_act_bwd_rows: [rows] pairs
 *     (sum dz, sum dz xh)); rstd = the forward's coef + 3 * rows.  Equal to torch's -(sum g w) u v^T / sigma. */
int gz_sn_sigma_coef_floats(int groups);      /* size of `coefs` (scratch) */
int gz_sn_sigma_term(const float* rowsums, const float* rstd, const float* sigma, const float* u, const float* v,
                     float* coefs, float* term, int rows, int groups, int R, int L, float eps, hipStream_t stream);
int gz_div_scalar(const float* x, const float* sigma, float* out, long long count, hipStream_t stream);
int gz_spectral_norm_bwd(const float* g, const float* rowdots, const float* u, const float* v, const float* sigma,
                         float* out, int R, int L, hipStream_t stream);

/* ---- normalisation + activation -------------------------------------------------------------
 * A tensor [N, C, inner] is N*C rows of `inner` contiguous floats (inner % 4 == 0).
 * coef layout: 4 arrays of `ncoef` floats (scale, shift, mean, rstd); ncoef = C for per-channel
 * statistics (BatchNorm), N*C for per-row statistics (InstanceNorm / AdaIN).
 * workspace: gz_norm_workspace_bytes(N, C) bytes.
 */
size_t gz_norm_workspace_bytes(int N, int C);
int gz_norm_coef_elems(int N, int C, int per_channel);

/* training-mode BatchNorm2d statistics (biased var for normalisation; running stats updated with the
 * unbiased var and `momentum`; *num_batches_tracked += 1).  Replaces the statistics half of
 * aten::native_batch_norm for nn.BatchNorm2d (standard_networks.py:44,87). */
/* the same from per-tile partials [rows][C][2] written by gz_conv2d_*_stats; count = elements per channel (N*H*W) */
int gz_batchnorm_finalize(const float* partials, int rows, long long count, const float* gamma, const float* beta,
                          float* coef, float* running_mean, float* running_var, long long* num_batches_tracked, int C,
                          float eps, float momentum, hipStream_t stream);
int gz_batchnorm_stats(const float* x, const float* gamma, const float* beta, float* coef, float* running_mean,
                       float* running_var, long long* num_batches_tracked, void* workspace, int N, int C,
                       int inner, float eps, float momentum, hipStream_t stream);
/* out[c] = sum over n and the inner dimension of x[n][c][:]: the bias gradient of a convolution (aten's
 * grad_bias); workspace as for the statistics passes (gz_norm_workspace_bytes) */
int gz_channel_sum(const float* x, float* out, void* workspace, int N, int C, int inner, hipStream_t stream);
/* eval-mode coefficients from the running statistics */
int gz_batchnorm_eval_coef(const float* gamma, const float* beta, const float* running_mean,
                           const float* running_var, float* coef, int C, float eps, hipStream_t stream);
/* per-row statistics: nn.InstanceNorm2d (standard_networks.py:46; gamma/beta per channel, biased var)
 * or AdaIN (hologan_generator.py:333-345; gamma/beta per row, unbiased var). */
int gz_rownorm_stats(const float* x, const float* gamma, const float* beta, float* coef, void* workspace, int N,
                     int C, int inner, float eps, int affine_per_row, int unbiased, hipStream_t stream);
/* gz_rownorm_stats + gz_norm_act_fwd(per_channel = 0) in one launch (the row is re-read from cache): coef as above,
 * out = act(x * scale + shift).  affine_per_row: 0 = gamma/beta per channel, 1 = per row ([N][C] arrays, AdaIN),
 * 2 = per row from one packed [N][2C] array (gamma = its base, beta = base + C: HoloGAN's ZMapping output,
 * hologan_generator.py:15-18). */
int gz_rownorm_act_fwd(const float* x, const float* gamma, const float* beta, float* coef, float* out, int N, int C,
                       int inner, float eps, int affine_per_row, int unbiased, int act, float slope,
                       hipStream_t stream);
/* AdaIN + activation of a constant shared by all samples (HoloGAN's learned 4^3 volume, hologan_generator.py:141
 * `self.x.repeat(batch, ...)`): x is [C][inner], sb the packed [N][2C] scale | shift, out / coef as for N*C rows.
 * Backward: dx [C][inner] (summed over the samples), dsb [N][2C]; inner <= 1024. */
int gz_adain_const_fwd(const float* x, const float* sb, float* coef, float* out, int N, int C, int inner, float eps,
                       int act, float slope, hipStream_t stream);
int gz_adain_const_bwd(const float* gout, const float* x, const float* coef, float* dx, float* dsb, int N, int C,
                       int inner, int act, float slope, hipStream_t stream);
/* out = act(x * scale + shift) */
int gz_norm_act_fwd(const float* x, const float* coef, float* out, int N, int C, int inner, int per_channel,
                    int act, float slope, hipStream_t stream);
/* first backward of norm+act: dx (may be NULL), dgamma, dbeta (may be NULL); kbuf: 2*ncoef floats scratch */
/* InstanceNorm (no affine) + activation with eps * sigma[n / (N / groups)]^2 per sample, and its first-order backward
 * that also leaves the row sums (sum dz, sum dz xh) in rowsums[N*C] pairs: the two halves of functional.sn_conv_in_act */
int gz_rownorm_act_fwd_sigma(const float* x, const float* sigma, int groups, float* coef, float* out, int N, int C,
                             int inner, float eps, int act, float slope, hipStream_t stream);
int gz_rownorm_act_bwd_rows(const float* gout, const float* x, const float* coef, float* dx, float* rowsums, int N, int C,
                            int inner, int act, float slope, hipStream_t stream);
int gz_norm_act_bwd(const float* gout, const float* x, const float* coef, float* dx, float* dgamma, float* dbeta,
                    void* workspace, float* kbuf, int N, int C, int inner, int per_channel, int affine_per_row,
                    int unbiased, int act, float slope, hipStream_t stream);
/* Round 4 -- BatchNorm with statistics GROUPS.  A discriminator step of the reference applies D to the real batch and
 * to the fake batch in two calls (core/lightning_module.py:112-119), each call normalising with its own batch
 * statistics and updating the running buffers.  Stacking the two batches along n and running ONE pass with groups = 2
 * is the same arithmetic -- group g = samples [g N/groups, (g+1) N/groups) has its own (scale, shift, mean, rstd) at
 * coef index g*C + c (coef holds 4 * groups * C floats), the running buffers are updated group after group,
 * num_batches_tracked += groups, dgamma / dbeta sum over the groups -- with half the launches and twice the rows per
 * launch.  `partials` of gz_batchnorm_finalize_g: rows of a convolution's fused statistics, the first rows/groups
 * belonging to group 0 etc. (the caller checks that no row straddles two groups); `count` = elements per group and
 * channel.  gz_batchnorm_act_bwd_g: accumulate != 0 adds the affine gradients to dgamma / dbeta (gradient sinks). */
int gz_batchnorm_stats_g(const float* x, const float* gamma, const float* beta, float* coef, float* running_mean,
                         float* running_var, long long* num_batches_tracked, void* workspace, int N, int C,
                         int inner, float eps, float momentum, int groups, hipStream_t stream);
int gz_batchnorm_finalize_g(const float* partials, int rows, long long count, const float* gamma, const float* beta,
                            float* coef, float* running_mean, float* running_var, long long* num_batches_tracked,
                            int C, float eps, float momentum, int groups, hipStream_t stream);
/* round 5: training-mode BatchNorm + activation forward with the finalize folded into the apply launch (one launch
 * when the producing convolution supplied `partials`; partials == NULL: row sums of x into `workspace` first) */
int gz_batchnorm_act_fwd_fused(const float* x, const float* partials, int rows, long long count, const float* gamma,
                               const float* beta, float* coef, float* running_mean, float* running_var,
                               long long* num_batches_tracked, void* workspace, float* out, int N, int C, int inner,
                               float eps, float momentum, int groups, int act, float slope, hipStream_t stream);
int gz_norm_act_fwd_g(const float* x, const float* coef, float* out, int N, int C, int inner, int per_channel,
                      int groups, int act, float slope, hipStream_t stream);
int gz_rownorm_act_bwd_acc(const float* gout, const float* x, const float* coef, float* dx, float* dgamma, float* dbeta,
                           void* workspace, float* kbuf, int N, int C, int inner, int act, float slope, int accumulate,
                           hipStream_t stream);       /* InstanceNorm(affine) first-order backward, same option */
int gz_batchnorm_act_bwd_g(const float* gout, const float* x, const float* coef, float* dx, float* dgamma, float* dbeta,
                           void* workspace, float* kbuf, int N, int C, int inner, int act, float slope, int groups,
                           int accumulate, hipStream_t stream);

/* backward of gz_norm_act_bwd's dx (per-row statistics, per-channel affine): given v = dL/d(dx) returns
 * gg_out = dL/d(gout), gx = dL/dx, ggamma = dL/dgamma (any may be NULL).  This is the InstanceNorm leg of
 * the gradient-penalty double backward (core/utils/utils.py:48-54 with create_graph=True). */
int gz_rownorm_act_bwd2(const float* gout, const float* v, const float* x, const float* coef, float* gg_out,
                        float* gx, float* ggamma, void* workspace, int N, int C, int inner, int act, float slope,
                        hipStream_t stream);
/* dx = g * act'(.) with the derivative expressed through the activation OUTPUT (LeakyReLU, ReLU, tanh) */
int gz_act_bwd(const float* g, const float* out, float* dx, long long count, int act, float slope,
               hipStream_t stream);
/* res = v * g * (-2 out): the derivative of gz_act_bwd's tanh result g * (1 - out^2) with respect to `out`, contracted
 * with v (second-order backward through a fused tanh epilogue) */
int gz_tanh_bwd2(const float* v, const float* g, const float* out, float* res, long long count, hipStream_t stream);

/* ---- row helpers (last discriminator layer, gradient-penalty tail, WGAN clip) -----------------
 * matrices are [R][L] row-major with L % 4 == 0. */
/* y[r] = sum_l a[r][l] * b[r][l]   (b_broadcast: b is a single row [L]) */
int gz_rowdot(const float* a, const float* b, float* y, int R, int L, int b_broadcast, hipStream_t stream);
/* out[r][:] = s[r] * x[r][:] (+ t[r] * x2[r][:], t = 1 - s when one_minus_s else s2); x_broadcast: x is [L] */
int gz_rowscale(const float* x, const float* s, const float* x2, const float* s2, float* out, int R, int L,
                int x_broadcast, int one_minus_s, hipStream_t stream);
/* ---- several small Linear layers over ONE input in one launch ------------------------------------------------
 * HoloGAN's five ZMapping layers, Linear(z_dim -> 2C) + ReLU each on the same z (core/models/hologan_generator.py:7-19,
 * called at :33/:57/:141).  table_host: gz_linear_multi_table_bytes() zeroed bytes of host memory filled through
 * gz_linear_multi_add (at most gz_linear_multi_max_jobs() layers; copied into the kernel argument).
 *   fwd: out_j[N][J_j] = act(x[N][K] . weight_j[J_j][K]^T + bias_j)          (g, dw, db unused: pass NULL)
 *   bwd: dw_j = (g_j * act'(out_j))^T . x,  db_j = its column sums (db NULL: skipped); weight/bias unused.
 * Any N, K, J (scalar loads); rows are summed in a fixed order. */
int gz_linear_multi_max_jobs(void);
size_t gz_linear_multi_table_bytes(void);
int gz_linear_multi_add(void* table_host, const float* weight, const float* bias, float* out, const float* g, float* dw,
                        float* db, int J);
int gz_linear_multi_fwd(void* table_host, const float* x, int N, int K, int act, float slope, hipStream_t stream);
int gz_linear_multi_bwd(void* table_host, const float* x, int N, int K, int act, float slope, hipStream_t stream);
/* out[l] = sum_r x[r][l]  (nn.Linear's bias gradient: core/models/hologan_discriminator.py:41-50, hologan_generator.py:11) */
int gz_colsum(const float* x, float* out, int R, int L, hipStream_t stream);
/* out[l] = sum_r g[r] * x[r][l] */
size_t gz_coldot_workspace_bytes(int R, int L);
int gz_coldot(const float* g, const float* x, float* out, float* workspace, size_t ws_bytes, int R, int L,
              hipStream_t stream);
/* gz_coldot without its slab sum (round 5): *nz_out row slices of L partial sums each are left in `workspace` (L floats
 * apart) for gz_reduce_multi / gz_adam_step_from_slabs; *nz_out == 1 means `out` is complete.  The critics' last layer
 * (Conv2d(8 f_d, 1, 4, 2, 0), reference standard_networks.py:27-30): its weight gradient joins the sinks unreduced. */
int gz_coldot_partial(const float* g, const float* x, float* out, float* workspace, size_t ws_bytes, int R, int L,
                      int* nz_out, hipStream_t stream);
/* dst[i] = src[i] for `words` 4-byte words; src may be PINNED HOST memory (device-mapped): the staging of the per-step
 * host draws -- `noise = distn.sample(...).to(device)`, core/lightning_module.py:107-108, core/utils/utils.py:41 */
int gz_copy_words(const void* src, void* dst, long long words, hipStream_t stream);
/* p = clamp(p, lo, hi) in place (core/lightning_module.py:160-162) */
int gz_clamp_(float* p, long long count, float lo, float hi, hipStream_t stream);

/* ---- R1-regularised ResNet path ------------------------------------------------------------
 * HBM-bound linear maps of reference core/submodules/gan_stability/models/resnet.py; every fwd/bwd pair is also
 * its own double-backward pair (the adjoint of the adjoint is the forward). count % 4 == 0. */
/* y = act(x): the pre-activation `actvn` (resnet.py:131-133) */
int gz_act_fwd(const float* x, float* y, long long count, int act, float slope, hipStream_t stream);
/* out = alpha*a + beta*b (b may be NULL); act_out (may be NULL) = act(out) written in the same pass:
 * the residual tail `x_s + 0.1*dx` (resnet.py:121-122) together with the next block's `actvn(x)` */
int gz_axpby(const float* a, float alpha, const float* b, float beta, float* out, float* act_out, long long count,
             int act, float slope, hipStream_t stream);
/* nn.AvgPool2d(3, stride=2, padding=1) (count_include_pad) over `planes` = N*C maps (resnet.py:72) and its
 * adjoint; OH = (H-1)/2 + 1 */
int gz_avgpool3s2_fwd(const float* x, float* y, long long planes, int H, int W, int OH, int OW, hipStream_t stream);
int gz_avgpool3s2_bwd(const float* gy, float* gx, long long planes, int H, int W, int OH, int OW,
                      hipStream_t stream);
/* nn.Upsample(scale_factor=2) (nearest, resnet.py:31) [planes,H,W] -> [planes,2H,2W] and its adjoint */
int gz_upsample2_fwd(const float* x, float* y, long long planes, int H, int W, hipStream_t stream);
int gz_upsample2_bwd(const float* gy, float* gx, long long planes, int H, int W, hipStream_t stream);

/* ---- input step ---------------------------------------------------------------------------------
 * decoded uint8 images [N,H,W,C] -> float [N,C,H,W] = (x / 255 - mean) / std: ToTensor() + Normalize(mean, std) of
 * core/lightning_module.py:42-47 on the device */
int gz_u8hwc_to_nchw(const unsigned char* in, float* out, int N, int H, int W, int C, float mean, float std,
                     hipStream_t stream);
/* the same step for a batch drawn from a uint8 set [M,H,W,C] that stays on the device:
 *   out[i,c,h,w] = (set[idx[i],h,w,c] / 255 - mean) / std,  labels_out[i] = labels[idx[i]]
 * for i < n, bit-equal to gz_u8hwc_to_nchw over the rows set[idx].  idx (int64 [n]) and labels (int64 [M], or NULL
 * together with labels_out) are device pointers; row byte offsets are 64-bit, so M*H*W*C is unbounded while n*H*W
 * < 2^31 (GZ_ERR_TOO_LARGE).  An idx[i] outside [0, M) is not dereferenced: row i of out is written as quiet NaN and
 * labels_out[i] as -1. */
int gz_u8hwc_gather_to_nchw(const unsigned char* set, long long M, const long long* idx, const long long* labels,
                            float* out, long long* labels_out, int n, int H, int W, int C, float mean, float std,
                            hipStream_t stream);

/* ---- DiffAugment of the discriminator's input (Zhao et al. 2020; csrc/gz_diffaug.hip) --------------
 * Per sample n of a batch [R0 + R1, C, H, W], with params[n] = {b, s, c, th, tw, h0, w0, unused} (fp32; the integers
 * stored as exact floats):
 *   x1 = x + b;  x2 = m + s (x1 - m), m = channel mean of x1 per pixel;  x3 = M + c (x2 - M), M = mean(x) + b;
 *   x4[., h, w] = x3[., h + th, w + tw] inside the image, else 0;  y = x4 with the box [h0, h0 + cut_h) x
 *   [w0, w0 + cut_w) zeroed (the box may lie partly outside the image; cut_h = cut_w = 0: no box).
 * y = A x + k with A = Mask . Shift . Con . Sat linear and k from b alone.  mode 0: A x + k; mode 1: A x (b ignored);
 * mode 2: A^T x = Con . Sat . Shift^T . Mask x (b ignored) -- the adjoint of modes 0/1, whose own adjoint is mode 1.
 * Rows [0, R0) are read from x0, rows [R0, R0 + R1) from x1 (x1 == NULL requires R1 == 0): the stacked discriminator
 * batch [aug(real); aug(fake)] is written by one launch without a concatenation copy.  params is [R0 + R1, 8], y is
 * [R0 + R1, C, H, W] and overlaps neither source.  One launch, no workspace, no atomics: every input element is read
 * once and every output element written once, the sample staying in registers in between; 16-byte stores wherever
 * the address is 16-byte aligned, any alignment of x0 / x1 / y to 4 bytes accepted.  The mean is a fixed-order
 * reduction (equal bits on every run) whose longest chain of dependent additions is 30.  A shift or corner outside
 * the image is clamped, never dereferenced.
 * Supported: 1 <= C <= 4, H, W >= 4, C*H*W <= 65536; anything else returns GZ_ERR_UNSUPPORTED and launches nothing.
 * GZ_ERR_BAD_SHAPE: a null x0 / params / y, x1 == NULL with R1 != 0, R0 or R1 negative, R0 + R1 < 1, a non-positive
 * dimension, a negative cut size, a mode outside 0..2, or y overlapping the rows read from x0 or x1. */
int gz_diffaug(const float* x0, const float* x1, const float* params, float* y, int R0, int R1, int C, int H, int W,
               int cut_h, int cut_w, int mode, hipStream_t stream);

/* ---- adaptive discriminator augmentation (Karras et al. 2020; csrc/gz_ada.hip) ------------------
 * gz_diffaug with a gate per sample and group and the two pixel-blitting transforms.  params is [R0 + R1, 16]:
 *   0..6   b, s, c, th, tw, h0, w0 as for gz_diffaug
 *   7      orientation code o = k + 4 f: f = x-flip bit, k = number of torch.rot90(., k, dims=[2, 3]) turns applied
 *          after the flip.  Clamped to [0, 7] (NaN: 0) and masked by `blit` (bit 0: x-flip permitted, bit 1: rot90
 *          permitted) inside the kernel
 *   8..12  uniforms in [0, 1) for the gates of color, translation, cutout, xflip, rot90
 *   13..15 zero (not read)
 * A group is ON iff p == NULL or u_group < p[0] (p: a device scalar).  Color off: the element passes through as
 * loaded, no colour arithmetic.  Translation off: shift (0, 0).  Cutout off: no box.  Xflip off or not permitted:
 * f = 0.  Rot90 off or not permitted: k = 0.  At p[0] = 0 all three modes return the input bits.
 *   A' = Mask . Shift . Q . Con . Sat,  Q x = rot90(flip_w(x) if f else x, k)  (a permutation commuting with Con . Sat)
 * mode 0: A' x + k; mode 1: A' x; mode 2: A'^T x = Con . Sat . Q^T . Shift^T . Mask x.  Sources, y, stacking, overlap
 * rule, alignment freedom and error codes as for gz_diffaug.  One launch, no workspace, no atomics.  The elements of
 * a sample are loaded in row-contiguous runs whatever the orientation and placed at their permuted positions in an
 * LDS plane (pitch W + 1 when k is odd), one channel at a time; samples with k even and no flip skip the staging.
 * The mean is a fixed-order reduction whose longest chain of dependent additions is 30.
 * Supported: the shapes of gz_diffaug; with bit 1 of blit set additionally H == W <= 128 (the staged plane of
 * H (W + 1) floats lives in LDS).  Anything else returns GZ_ERR_UNSUPPORTED and launches nothing.
 * GZ_ERR_BAD_SHAPE: as for gz_diffaug, or blit outside 0..3. */
int gz_diffaug_gated(const float* x0, const float* x1, const float* params, const float* p, float* y, int R0, int R1,
                     int C, int H, int W, int cut_h, int cut_w, int blit, int mode, hipStream_t stream);
/* The ADA controller.  state = four device floats {sum_sign, count, p, last_r}; nothing synchronises with the host.
 * gz_ada_observe: state[0] += sum_i sign(logits[i]), sign = (x > 0) - (x < 0) (NaN and +-0 contribute 0);
 *   state[1] += n.  One workgroup, fixed order: exact integers in fp32 below 2^24.
 * gz_ada_update: if state[1] > 0: r = state[0] / state[1]; p = min(max(p + step * sgn(r - target), 0), 1);
 *   state[3] = r; state[0] = state[1] = 0.  Otherwise nothing changes.
 * GZ_ERR_BAD_SHAPE: a null pointer, n < 1, a non-finite or negative step, a non-finite target. */
int gz_ada_observe(const float* logits, int n, float* state, hipStream_t stream);
int gz_ada_update(float* state, float target, float step, hipStream_t stream);

/* ---- fused multi-tensor optimizer steps (the `optimiser` nodes of conf/expt/<name>.yaml) -------------------------
 * `count` <= GZ_OPT_MAX_TENSORS tensors per call (host arrays of device pointers and element counts);
 * grads are multiplied by grad_scale first (1/world for data-parallel means).  Formulas are torch.optim's
 * single-tensor ones (no weight decay, no amsgrad / momentum / centered).
 * zero_grads != 0: every gradient element is overwritten with 0 after it has been read -- the zero_grad(set_to_none=
 * False) of the reference's harness in the same pass (the flat data-parallel exchange buffer must read zero again). */
#define GZ_OPT_MAX_TENSORS 24
int gz_adam_step(int count, float* const* params, float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq, const long long* numel, float lr, float beta1, float beta2, float eps,
                 int step, float grad_scale, int zero_grads, hipStream_t stream);
/* Adam reading UNREDUCED weight-gradient slabs (gz_conv2d_wgrad_partial) instead of a gradient tensor: the slab sum of
 * gz_reduce_multi and the update in one launch (harness.Trainer outside data parallelism).  A zero-initialised host
 * table of gz_adam_src_table_bytes() bytes takes <= gz_adam_src_max_tensors() parameters with <= 4 sources each
 * (gz_adam_src_add per (parameter, source)); the gradient has the bits gz_reduce_multi would have written. */
int gz_adam_src_max_tensors(void);
size_t gz_adam_src_table_bytes(void);
int gz_adam_src_add(void* table_host, float* param, float* exp_avg, float* exp_avg_sq, long long numel,
                    const float* slabs, int nz, long long stride);
int gz_adam_step_from_slabs(void* table_host, float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                            hipStream_t stream);
/* graph-capturable Adam: tick = device float[3] {step, 1 - beta1^step, sqrt(1 - beta2^step)}; gz_adam_tick advances
 * it by one step, gz_adam_step_dev reads the corrections from it (same update as gz_adam_step) */
int gz_adam_tick(float* tick, float beta1, float beta2, hipStream_t stream);
int gz_adam_step_dev(int count, float* const* params, float* const* grads, float* const* exp_avg,
                     float* const* exp_avg_sq, const long long* numel, float lr, float beta1, float beta2, float eps,
                     const float* tick, float grad_scale, int zero_grads, hipStream_t stream);
int gz_rmsprop_step(int count, float* const* params, float* const* grads, float* const* square_avg,
                    const long long* numel, float lr, float alpha, float eps, float grad_scale, int zero_grads,
                    hipStream_t stream);

/* ---- generator weight averaging (reference core/submodules/gan_stability/train.py:144-153, update_average) ---------
 * avg[i] = beta * avg[i] + one_minus_beta * src[i] over ANY number of tensors in one launch: two multiplies and one
 * add per element without FMA contraction, the same bits on the float4 path (both arrays of a job 16-byte aligned), the
 * scalar path and under any split of the tensors over launches.  The job table lives in DEVICE memory and is built
 * once (gz_conv2d_pack_multi's pattern): gz_ema_job fills one host-side record of gz_ema_job_bytes() bytes with the
 * pair, its element count and first_block = the sum of the block counts returned for the jobs in front of it, and
 * returns the job's own block count (>= 0; a numel == 0 job has none, is skipped by the launch and may carry null
 * pointers) or GZ_ERR_BAD_SHAPE for a null pointer, a negative numel / first_block or overlapping avg / src ranges;
 * it touches no device.  gz_ema_update launches over `count` jobs copied to jobs_dev and total_blocks = the sum of
 * their block counts (0 launches nothing); beta travels by value, so a captured launch replays.  The caller computes
 * one_minus_beta as (float)(1.0 - (double)beta), which is what torch makes of the reference's `(1. - beta)`. */
size_t gz_ema_job_bytes(void);
int gz_ema_job(void* job_out, float* avg, const float* src, long long numel, int first_block);
int gz_ema_update(const void* jobs_dev, int count, int total_blocks, float beta, float one_minus_beta,
                  hipStream_t stream);

/* ---- KID on the device (reference core/callback_inception_metrics.py:15-133) ----------------------------------------
 * Everything `_mmd2_and_variance` reads of the three polynomial-kernel matrices of S subsets, in fp64 on
 * v_mfma_f64_16x16x4_f64, without a kernel matrix in memory.  codes_g [n_g, d] and codes_r [n_r, d] are fp64 row-major
 * DEVICE arrays, idx [S][2][m] int32 DEVICE row numbers into codes_g (slot 0) and codes_r (slot 1), gathered on load.
 * With G = codes_g[idx[s][0]], R = codes_r[idx[s][1]] and K_AB = (gamma * A B^T + coef0)^degree (repeated
 * multiplication, degree >= 1), out [S][6*m + 3] receives per subset
 *     rowsum(K_GG) (diagonal included) | diag(K_GG) | rowsum(K_RR) | diag(K_RR) | rowsum(K_GR) | colsum(K_GR) |
 *     |K_GG|_F^2, |K_RR|_F^2, |K_GR|_F^2.
 * d and m need no multiple of anything.  Deterministic: no floating-point atomics, a fixed order for every sum, and
 * neither `out` nor the workspace (gz_kid_workspace_bytes bytes) has to be zeroed.  Two launches on `stream`.
 * GZ_ERR_BAD_SHAPE: S, m, d, degree, n_g or n_r below 1, m > min(n_g, n_r), a null pointer; GZ_ERR_WORKSPACE: workspace
 * too short (nothing is launched).  The index VALUES are the caller's contract: they are not checked here. */
size_t gz_kid_workspace_bytes(int S, int m, int d);
int gz_kid_sums(const double* codes_g, int n_g, const double* codes_r, int n_r, int d, const int* idx, int S, int m,
                double gamma, double coef0, int degree, double* out, void* workspace, size_t ws_bytes,
                hipStream_t stream);

/* ---- activation statistics on the device (reference core/callback_inception_metrics.py:223-231) -----------------------
 * mean [d] and cov [d][d] = np.cov(act, rowvar=False) of act [n][d], fp64 row-major DEVICE arrays, on
 * v_mfma_f64_16x16x4_f64 (csrc/gz_moments.hip).  numpy's two-pass form in numpy's order: column means, c = x - mean as
 * the values are loaded, cov = (C^T C) * (1.0 / (n - 1)).  n and d need no multiple of anything; row offsets are 64-bit.
 * Deterministic: no floating-point atomics, a fixed order for every sum, and neither the outputs nor the workspace
 * (gz_feature_moments_workspace_bytes bytes) has to be zeroed; two calls give equal bits, and cov[i][j] and cov[j][i]
 * are the same bits (upper-triangle tiles, mirrored by the epilogue).  Three launches on `stream`.
 * GZ_ERR_BAD_SHAPE: n < 2, d < 1, a null pointer; GZ_ERR_WORKSPACE: workspace too short (nothing is launched). */
size_t gz_feature_moments_workspace_bytes(long long n, int d);
int gz_feature_moments(const double* act, long long n, int d, double* mean, double* cov, void* workspace,
                       size_t ws_bytes, hipStream_t stream);

/* ---- matrix square root on the device: the Newton-Schulz primitives (csrc/gz_sqrtm.hip) --------------
 * gz_sqrtm_product: C = alpha * (A B) + beta * I for fp64 row-major d x d DEVICE matrices on v_mfma_f64_16x16x4_f64, one
 * workgroup per 64 x 64 tile of C with the whole reduction index inside it.  Nothing is assumed about symmetry; d needs
 * no multiple of anything (indices >= d are never dereferenced).  C must not overlap A or B; A and B may be one matrix.
 * gz_sqrtm_product_pair: two such products of one size in ONE launch (the iteration's Y T and T Z), each with its own
 * operands and coefficients; neither output may overlap any of the four operands or the other output.
 * Deterministic: no floating-point atomics, every entry summed over k in k order, C is written and never read; two calls
 * give equal bits.  No workspace.  The launcher neither synchronises nor allocates: one launch on `stream`.
 * GZ_ERR_BAD_SHAPE: d < 1, a null pointer, an output that overlaps an operand or the other output (nothing is launched).
 *
 * gz_sqrtm_trace_norm: out[0] = trace(A), out[1] = |A|_F^2 (the sum of the squared entries) of a d x d DEVICE matrix into
 * two DEVICE doubles, in a fixed order: 8 rows per workgroup into the workspace (gz_sqrtm_trace_norm_workspace_bytes
 * bytes, never read before it is written), then the workgroups' shares in workgroup order.  Two launches on `stream`.
 * GZ_ERR_BAD_SHAPE: d < 1, a null pointer; GZ_ERR_WORKSPACE: workspace too short (nothing is launched). */
int gz_sqrtm_product(const double* a, const double* b, double* c, int d, double alpha, double beta,
                     hipStream_t stream);
int gz_sqrtm_product_pair(const double* a0, const double* b0, double* c0, double alpha0, double beta0,
                          const double* a1, const double* b1, double* c1, double alpha1, double beta1, int d,
                          hipStream_t stream);
size_t gz_sqrtm_trace_norm_workspace_bytes(int d);
int gz_sqrtm_trace_norm(const double* a, int d, double* out, void* workspace, size_t ws_bytes, hipStream_t stream);

/* ---- Inception Score on the device (csrc/gz_inception_score.hip) ---------------------------------------
 * The statistic of the reference's core/submodules/gan_stability/metrics/inception_score.py on the classifier head that
 * the FID weight file carries (NOT torchvision's ImageNet network, which the reference runs a second time).
 * gz_classifier_logits: logits[i][c] = sum_k codes[i][k] weight[c][k] + bias[c] for fp64 row-major DEVICE arrays codes
 * [n][d], weight [classes][d] (nn.Linear's layout), bias [classes] (may be null), logits [n][classes], on
 * v_mfma_f64_16x16x4_f64, one workgroup per 64 x 64 tile with the whole reduction index inside it.  n, d and classes need
 * no multiple of anything (indices outside are never dereferenced); row offsets are 64-bit.  Every entry is summed over k
 * in k order; logits is written and never read; no workspace; one launch on `stream`.
 * GZ_ERR_BAD_SHAPE: n, d or classes below 1, a null pointer (bias excepted), logits overlapping codes or weight;
 * GZ_ERR_TOO_LARGE: more than 2^31 - 1 tiles, or an array beyond the address space (nothing is launched).
 *
 * gz_inception_score: scores[s] = exp(mean_i sum_c p_ic (log p_ic - log py_c)) for s < splits into `splits` DEVICE doubles,
 * where split s is rows s (n / splits) .. (s + 1) (n / splits) - 1 of logits [n][classes] (the trailing n % splits rows are
 * ignored), p_i = softmax(logits_i) stabilised by the row maximum and py = mean_i p_i over the split.  A class with p = 0
 * contributes 0, as in scipy.stats.entropy; logits of +-800 give no NaN; a split of one row scores exactly 1.  classes has
 * no cap (no row is kept in LDS).  Deterministic: no floating-point atomics, every sum in a fixed order (rows in order
 * inside a block of 64 rows that never spans two splits, blocks in block order), neither `scores` nor the workspace
 * (gz_inception_score_workspace_bytes bytes: two doubles per row, one double per class and block of 64 rows) has to be
 * zeroed; two calls give equal bits.  Five launches on `stream`.
 * GZ_ERR_BAD_SHAPE: n, classes or splits below 1, splits > n, a null pointer; GZ_ERR_TOO_LARGE: a grid beyond 2^31 - 1
 * workgroups; GZ_ERR_WORKSPACE: workspace too short (nothing is launched; the size query returns 0 for a refused shape). */
int gz_classifier_logits(const double* codes, long long n, int d, const double* weight, const double* bias,
                         int classes, double* logits, hipStream_t stream);
size_t gz_inception_score_workspace_bytes(long long n, int classes, int splits);
int gz_inception_score(const double* logits, long long n, int classes, int splits, double* scores,
                       void* workspace, size_t ws_bytes, hipStream_t stream);

/* ---- precision / recall / density / coverage on the device (csrc/gz_prdc.hip) ---------------------------
 * The k-nearest-neighbour manifold metrics (improved precision and recall, Kynkaanniemi et al. 2019; density and coverage,
 * Naeem et al. 2020) of fp64 row-major DEVICE codes, on SQUARED Euclidean distances in the Gram form
 * D(x, y) = max(0, |x|^2 + |y|^2 - 2 <x, y>) on v_mfma_f64_16x16x4_f64, without a distance matrix in memory.  All
 * comparisons are <=.  n, n_g, n_r and d need no multiple of anything (an index outside an operand is never
 * dereferenced); row offsets are 64-bit.
 *
 * gz_knn_radii: radii[i] = the k-th smallest of D(codes_i, codes_j) over j != i (self excluded by index: exact duplicates
 * give 0) into n DEVICE doubles, 1 <= k <= 8, k < n.  Selection by value: the same bits for every slicing of the walk.
 * Three launches on `stream`.
 *
 * gz_prdc_counts: one walk over the n_g x n_r cross distances, each tile computed once, with rad_g [n_g] and rad_r [n_r]
 * (gz_knn_radii's, or any DEVICE doubles):
 *     in_real[j] = #{i : D(G_j, R_i) <= rad_r[i]}   int32 [n_g]        in_fake[i] = #{j : D(G_j, R_i) <= rad_g[j]}   int32 [n_r]
 *     near[i]    = min_j D(G_j, R_i)                double [n_r]
 *     totals     = #{in_real > 0}, #{in_fake > 0}, sum in_real, #{near <= rad_r}                     int64 [4]
 * so that precision = totals[0] / n_g, recall = totals[1] / n_r, density = totals[2] / (k n_g), coverage = totals[3] / n_r.
 * Five launches on `stream`.
 *
 * gz_prdc_plan: the grid gz_prdc_counts takes for n_rows generated and n_cols real rows at the current CU budget
 * (gz_set_cu_budget): row_groups groups of row tiles (at most 128, equal up to one tile) times col_slices slices of column
 * tiles (as many as fit with them into one round of two workgroups per CU, at most one per column tile).  It depends on
 * nothing else.  gz_knn_radii of n rows takes the plan of (n, n).
 *
 * Deterministic: no atomics, every count an integer sum and near a minimum, and neither the outputs nor the workspaces
 * (gz_knn_radii_workspace_bytes / gz_prdc_counts_workspace_bytes bytes) have to be zeroed; two calls give equal bits.
 * GZ_ERR_BAD_SHAPE: k < 1, k > 8, k >= n, n_g, n_r or d below 1, a null pointer; GZ_ERR_TOO_LARGE: a grid beyond 2^31 - 1
 * workgroups or an array beyond the address space; GZ_ERR_WORKSPACE: workspace too short (nothing is launched; the size
 * queries return 0 for a refused shape). */
size_t gz_knn_radii_workspace_bytes(long long n, int d, int k);
int gz_knn_radii(const double* codes, long long n, int d, int k, double* radii, void* workspace, size_t ws_bytes,
                 hipStream_t stream);
size_t gz_prdc_counts_workspace_bytes(long long n_g, long long n_r, int d);
int gz_prdc_counts(const double* codes_g, long long n_g, const double* rad_g, const double* codes_r, long long n_r,
                   const double* rad_r, int d, int* in_real, int* in_fake, double* near, long long* totals,
                   void* workspace, size_t ws_bytes, hipStream_t stream);
int gz_prdc_plan(long long n_rows, long long n_cols, int* row_groups, int* col_slices);

/* ---- sliced Wasserstein distance on Laplacian-pyramid patches (csrc/gz_swd.hip) ------------------------
 * The metric of Karras et al. 2018 (section 5 and appendix) from pixels alone: eval.swd is the definition, eval.swd_device
 * strings these launchers together.  All of them: fp32 (statistics and sums fp64) DEVICE arrays, wave64 vector code, no
 * atomics, every sum in a fixed order, no output or workspace read before this call wrote it: two calls give equal bits.
 * No launcher allocates or synchronises.
 *
 * gz_swd_pyramid: x [N][C][S][S] -> the Laplacian levels S, S/2, .., 16 packed into out: level l is [N][C][S_l][S_l] at
 * float offset offsets[l] (gz_swd_pyramid_describe: levels, offsets[0 .. levels], the last one the total).  down: the
 * 5 taps [1,4,6,4,1]/16 along W, then along H, mirror border (-1 -> 1, n -> n - 2), even rows and columns; up: zeros at the
 * odd positions, the same taps * 2 along H, then along W; L_l = G_l - up(G_l+1), the coarsest level is G itself.  Each tap
 * sum runs t = 0 .. 4 in order.  One workgroup per plane keeps every level of it in LDS (127 KiB at S = 128): x is read once,
 * each level written once.  One launch.  GZ_ERR_UNSUPPORTED: S not in {16, 32, 64, 128}; GZ_ERR_BAD_SHAPE: N < 1, C not 1
 * or 3, a null pointer; GZ_ERR_WORKSPACE: out_elems below the total.
 *
 * Patches: pos [rows][2] int32 holds (cy, cx) of row r = image * P + patch, rows = n * P, centres in [3, H - 3) (a centre
 * outside is clamped into it, never dereferenced outside the plane).  Descriptor element k = (c * 7 + dy) * 7 + dx is
 * level[image][c][cy - 3 + dy][cx - 3 + dx], D = 49 C.
 *
 * gz_swd_channel_stats: stats[c] = mean, stats[C + c] = population standard deviation of channel c over the rows * 49
 * gathered values, 2 C doubles.  Sums of v - v0 and (v - v0)^2 in fp64, v0 = the channel's first gathered value (row 0, tap
 * 0), so that a constant channel gives a standard deviation of exactly 0: thread-strided rows, the xor butterfly, waves in
 * order, workgroups in order.  Two launches; workspace gz_swd_channel_stats_workspace_bytes.
 *
 * gz_swd_project: proj[j][r] = sum_k x_rk dirs[j][k] for j < ndirs, r < rows, with x_rk = (d_rk - (float)mean_c) *
 * (float)(1 / std_c) (std_c == 0 divides by 1) from stats as gz_swd_channel_stats writes it.  fp32, in this order: the 7 products
 * of one patch row (c, dy) form one chain of fused multiply-adds from 0, dx ascending; the 7 C chain results are added to
 * one total in (c, dy) order -- 7 + 7 C roundings on any path, which the tests' error bound rests on.  Descriptors never
 * reach memory: a workgroup gathers 128 rows
 * into LDS beside 128 directions (147 KiB).  proj has row pitch `pitch` >= the sort's padded length (gz_swd_sort_plan);
 * entries rows .. padded - 1 of every direction are set to +inf, entries beyond are not touched.  One launch.
 *
 * gz_swd_sort_columns: every one of `cols` arrays data[j * pitch + 0 .. rows - 1] ascending, in place, by a bitonic
 * network on the keys' bits mapped to order-preserving integers (-0.0 below +0.0, no NaN handling).  Entries rows ..
 * padded - 1 come out +inf whatever they held; entries padded .. pitch - 1 are not touched.  A block pass sorts or merges
 * `block` keys in one workgroup (strides below 16 in registers, 16 .. 512 by lane exchange, above through LDS); a global
 * pass is one compare-exchange stride >= block, or two of them fused (a phase's strides go two to a pass while two are
 * left), with 16-byte accesses.  gz_swd_sort_plan: block, padded = the power of two >= rows,
 * and the number of block and global passes (launches).  pitch % 4 == 0 and data 16-byte aligned.
 *
 * gz_swd_distance: out[q] = sum over the columns q * cols_per_repeat .. (q + 1) * cols_per_repeat - 1 and rows of
 * |a - b| in fp64 (the caller divides by rows * cols_per_repeat), q < repeats.  Thread-strided rows of one column per
 * workgroup and row chunk, butterfly, waves in order, then the chunks and columns of a repeat in order.  Two launches;
 * workspace gz_swd_distance_workspace_bytes.  GZ_ERR_BAD_SHAPE: rows_a != rows_b.
 *
 * Everywhere: GZ_ERR_BAD_SHAPE for a count below 1 (P = 0 included), a null pointer, a pitch below the padded length;
 * GZ_ERR_TOO_LARGE for a grid beyond 2^31 - 1; GZ_ERR_WORKSPACE for a short workspace.  A refused call launches nothing;
 * the size queries return 0 for a refused shape. */
int gz_swd_pyramid_describe(int N, int C, int S, int* levels, long long* offsets);
int gz_swd_pyramid(const float* x, int N, int C, int S, float* out, long long out_elems, hipStream_t stream);
size_t gz_swd_channel_stats_workspace_bytes(int n, int C, int H, int P);
int gz_swd_channel_stats(const float* level, int n, int C, int H, const int* pos, int P, double* stats,
                         void* workspace, size_t ws_bytes, hipStream_t stream);
int gz_swd_project(const float* level, int n, int C, int H, const int* pos, int P, const double* stats,
                   const float* dirs, int ndirs, float* proj, long long pitch, hipStream_t stream);
int gz_swd_sort_plan(long long rows, int* block, long long* padded, int* block_passes, int* global_passes);
int gz_swd_sort_columns(float* data, long long rows, int cols, long long pitch, hipStream_t stream);
size_t gz_swd_distance_workspace_bytes(long long rows, int cols_per_repeat, int repeats);
int gz_swd_distance(const float* a, long long rows_a, const float* b, long long rows_b, int cols_per_repeat, int repeats,
                    long long pitch, double* out, void* workspace, size_t ws_bytes, hipStream_t stream);

/* text of the last HIP error seen by a launcher on the calling thread ("" if none) */
const char* gz_last_error(void);

/* library identification: returns the gfx target string the kernels were compiled for */
const char* gz_build_info(void);
/* content digest (sha256 prefix, hex) of the kernel sources, headers and flags this library was built from;
 * lightning_gan_zoo_amd/_lib.py refuses a library whose digest is not the digest of the tree it runs from */
const char* gz_source_digest(void);

#ifdef __cplusplus
}
#endif
#endif /* GZ_OPS_H */
