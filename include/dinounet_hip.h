/*
 * dinounet_hip.h -- C ABI of libdinounet_hip.so: the MI355X (gfx950) kernels behind the Dino U-Net
 * forward/backward hot path.  Plain pointers and sizes only (no torch types); every entry point
 * enqueues on the caller's HIP stream, does not synchronise, keeps no global state and returns 0 on
 * success or a negative DU_ERR_* code (the Python host turns that into RuntimeError, mirroring the
 * AT_ASSERTM behaviour of the reference extension, ops/src/cuda/ms_deform_attn_cuda.cu:33-57).
 *
 * All pointers are DEVICE pointers unless stated otherwise.  Conv-side tensors are NHWC ("pixel-major",
 * channel-contiguous); token tensors are (B, N, D) row-major -- the same memory as NHWC.  `ld*` are row
 * (pixel) strides in ELEMENTS, so a channel slice of a wider NHWC tensor can be read/written in place.
 *
 * Reference interfaces replaced (paths relative to the reference root):
 *   du_msda_forward / du_msda_backward
 *       <- ms_deform_attn_forward / ms_deform_attn_backward, the two pybind names of the extension
 *          `MultiScaleDeformableAttention` (ops/src/vision.cpp:18-21, ops/src/ms_deform_attn.h:25-66,
 *          kernels ops/src/cuda/ms_deform_im2col_cuda.cuh:242-304 and :961-1332)
 *   du_gemm (linear / 1x1 conv / implicit 3x3 conv / transposed conv, fwd + dgrad + wgrad)
 *       <- torch F.linear / F.conv2d / F.conv_transpose2d call sites: layers/attention.py:88-90,
 *          layers/ffn_layers.py:43-49, layers/patch_embed.py:70, ms_deform_attn.py:183-215,
 *          dinov3_adapter.py:85-89,239-277,360,467, dinounet_training.py:423-438,253,613-619
 *   du_attention_fwd, du_qkv_rope_split
 *       <- SelfAttention.compute_attention / apply_rope (layers/attention.py:66-85,106-118)
 *   du_layernorm_fwd / _bwd      <- nn.LayerNorm (layers/block.py:43,56; dinov3_adapter.py:128-137)
 *   du_chan_stats / du_norm_act_* <- InstanceNorm2d+LeakyReLU (dinounet_training.py:401,238; decoder
 *          StackedConvBlocks :581-592) and SyncBatchNorm(+ReLU) (dinov3_adapter.py:242-270,361-364)
 *   du_dwconv3x3_fwd / _bwd      <- DWConv (dinov3_adapter.py:94-109), DepthwiseSeparableConv.depthwise
 *          (dinounet_training.py:235): one call per pass; the library picks the band kernels (dwconv.hip: a workgroup walks
 *          a band of rows, GELU backward fused into the data gradient) or the row kernels (elementwise.hip) by the plan
 *          of csrc/dwconv_plan.h; du_dwconv3x3_plan_describe reports that plan
 *   du_maxpool3x3s2_*            <- nn.MaxPool2d(3,2,1) (dinov3_adapter.py:250)
 *   du_bilinear_add_*            <- F.interpolate(bilinear, align_corners=False)+add (dinov3_adapter.py:472-476)
 *   du_se_gate_* / du_se_scale_*  <- SqueezeExcitation + residual (dinounet_training.py:210-225,438)
 *   du_msda_prep / du_msda_prep_bwd <- ms_deform_attn.py:188-197
 *   du_dice_ce_*                  <- DC_and_CE_loss (training/loss/compound_losses.py:8-56, dice.py:58-119), the loss nnUNetTrainer.train_step
 *          applies to the logits (nnUNetTrainer.py:917); "next" row of the scope table
 *   du_ds_loss_*, du_downsample_seg <- DeepSupervisionWrapper (training/loss/deep_supervision.py) with the weights of
 *          nnUNetTrainer._build_loss (nnUNetTrainer.py:373-387) and DownsampleSegForDSTransform2 (deep_supervision_donwsampling.py)
 *   du_dice_ce_masked_*, du_dice_bce_*, du_labels_to_regions
 *       <- the ignore-label and region configurations of nnUNetTrainer._build_loss (nnUNetTrainer.py:355-365):
 *          DC_and_CE_loss(ignore_label) (compound_losses.py:31-56), DC_and_BCE_loss (compound_losses.py:83-99),
 *          ConvertSegmentationToRegionsTransform (nnUNetTrainer.py:766-767)
 *   du_topk_loss_*                <- TopKLoss (training/loss/robust_ce_loss.py:19-32), DC_and_topk_loss (compound_losses.py:102-150)
 *   du_export_seg, du_seg_counts
 *       <- convert_predicted_logits_to_segmentation_with_correct_shape (inference/export_prediction.py:15-68) and
 *          compute_metrics' counts (evaluation/evaluate_predictions.py:75-94, 176-186)
 *   du_ensemble_merge
 *       <- average_probabilities and merge_files (ensembling/ensemble.py:17-46)
 *   du_surface_border, du_surface_field, du_surface_gather
 *       <- compute_surface_distances (evaluation/evaluate_predictions.py:97-149): medpy.metric.hd95 / asd, restated
 */
#ifndef DINOUNET_HIP_H
#define DINOUNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DU_OK 0
#define DU_ERR_BAD_ARG (-1)
#define DU_ERR_UNSUPPORTED (-2)
#define DU_ERR_LAUNCH (-3)

/* element types */
#define DU_F32 0
#define DU_BF16 1

/* du_gemm operand addressing modes.  The logical product is C[m][n] = sum_k A(m,k) * B(n,k). */
#define DU_PLAIN_ROW 0   /* element (outer o, contraction k) at p[o*ld + k]          (k contiguous) */
#define DU_PLAIN_COL 1   /* element (outer o, contraction k) at p[k*ld + o]          (o contiguous) */
#define DU_IM2COL_ROW 2  /* outer = output pixel, contraction = (tap, channel) gathered from an NHWC tensor */
#define DU_IM2COL_COL 3  /* outer = (tap, channel), contraction = pixel (used by conv weight gradients) */

/* du_gemm epilogue activations */
#define DU_ACT_NONE 0
#define DU_ACT_GELU 1    /* exact erf GELU (nn.GELU default) */
#define DU_ACT_RELU 2
#define DU_ACT_LEAKY 3   /* LeakyReLU(0.01) */
#define DU_ACT_SWIGLU 4  /* gate of SwiGLUFFN (layers/ffn_layers.py:73-77) on an INTERLEAVED projection: B rows (2j, 2j+1) = (w1[j], w2[j]),
                            bias likewise; the result has N/2 columns, C[m][j] = silu(v[2j]) * v[2j+1], v = alpha*acc + bias; ldc / the
                            stored row length refer to those N/2 columns.  Served by the multi-phase bf16 NT kernels only (du_gemm
                            returns DU_ERR_UNSUPPORTED otherwise: run the product without activation + du_swiglu_pairs) */

/* du_gemm store modes */
#define DU_STORE_PLAIN 0
#define DU_STORE_SLABS 4 /* split_k > 1, fp32 result, generic bf16 engine only: split s writes its partial product with plain stores to
                            C + s * M * ldc (split_k slabs of M x ldc floats, no zero fill needed) instead of adding into C atomically --
                            the caller reduces the slabs in a fixed order (du_splitk_reduce_bf16): bit-reproducible results */
#define DU_STORE_QKV_HEADS 5 /* as DU_STORE_QKV_ROPE without the rotation and the q scale: the projection (+ bias) stored head-major in the
                               three planes (ps_H / ps_W / ps_C as there), rotated afterwards where it lies by du_qkv_rope_inplace.  Served by the
                               persistent multi-phase kernel only (K >= 384; M % 256 == 0, or 1 .. 64 rows behind the last full 256-row tile, which ride in
                               the same launch: du_gemm_plan_describe's tail_rows; DU_ERR_UNSUPPORTED otherwise) */
#define DU_STORE_MSDA_PREP 6 /* MSDeformAttn's sampling_offsets | attention_weights product (ms_deform_attn.py:188-197) with the reference-point /
                               softmax step in the epilogue: N = heads * 12 columns = [heads x 4 points x (x, y) offsets | heads x 4 logits] (+ bias),
                               fp32; instead of the matrix, C receives the sampling locations (M, heads, 4, 2) = ref[m % ps_C] + offset / (ps_W,
                               ps_H) and C2 the softmax over the 4 points (M, heads, 4); rope_sin = ref (ps_C, 2) fp32.  Served by the 256 x 256
                               multi-phase kernel only (N <= 256, K % 128 == 0; DU_ERR_UNSUPPORTED otherwise: du_msda_prep on the plain result) */
#define DU_STORE_TAPS 3 /* grouped convolution weight gradients only (du_gemm_tn_group: du_tn_job.taps): column n = (tap, c) of the product is
                           element (m, c, tap) of a torch-layout weight gradient */
#define DU_STORE_QKV_ROPE 2 /* the ViT's qkv projection stored head-major with RoPE: row m = (b, token t) of M = B * ps_H tokens, column
                              n = (which, h, d) of N = 3 * ps_C * 64 -> out[which][b][h][t][d] in three (B, ps_C, ps_W = Npad, 64) planes ldc
                              elements apart; q and k of tokens >= rope_prefix are rotated (rotate-half, fp32) with rope_sin / rope_cos
                              ((ps_H - prefix, 64) fp32), q is multiplied by rope_qscale.  bf16, d_head 64, bias-only epilogue; served
                              by the 256 x 128 multi-phase kernel only (DU_ERR_UNSUPPORTED otherwise: du_qkv_rope_split then) */
#define DU_STORE_PIXEL_SHUFFLE2 1 /* ConvTranspose2d k2 s2: column n=(dy*2+dx)*Cout+co of input pixel (b,y,x)
                                     goes to output pixel (b,2y+dy,2x+dx), channel co */

typedef struct {
  /* source NHWC tensor(s): channels [0,C1) come from p (pixel stride ld), channels [C1,C) from p2 (ld2).
     This is how the decoder's torch.cat (dinounet_training.py:614) is consumed without materialising it. */
  const void* p2;
  int64_t ld2;
  int32_t C1;
  int32_t Hi, Wi;      /* source spatial size */
  int32_t C;           /* total gathered channels (C1 + C2) */
  int32_t KH, KW, stride, pad;
  int32_t Ho, Wo;      /* grid the "pixel" index runs over */
  int32_t transposed;  /* 0: yi = yo*stride - pad + dy.  1: yi = (yo + pad - dy)/stride when divisible (dgrad) */
} du_conv_geom;

typedef struct {
  int32_t dtype;      /* DU_F32 / DU_BF16: element type of A and B */
  int32_t out_dtype;  /* element type of C and residual */
  int32_t a_mode, b_mode;
  int32_t M, N, K;
  const void* A; int64_t lda; int64_t a_batch_stride;
  const void* B; int64_t ldb; int64_t b_batch_stride;
  void* C; int64_t ldc; int64_t c_batch_stride;
  int32_t batch;      /* >= 1 */
  int32_t split_k;    /* >= 1; > 1 requires out_dtype F32, a zero-initialised C and no epilogue ops */
  float alpha;
  const float* bias;  /* [N] fp32 or NULL */
  int32_t act;
  const float* gamma; /* [N] fp32 or NULL: per-column scale applied after act (LayerScale) */
  const float* row_scale; int32_t rs_rows; /* optional per-row-block scale v *= row_scale[m / rs_rows] (DropPath) */
  const void* residual; int64_t ldr; /* added last, NULL for none; may alias C.  Indexed like C: with DU_STORE_PIXEL_SHUFFLE2 it is a
                                        tensor of the OUTPUT shape (pixel stride ldr), e.g. the skip added to a ConvTranspose result */
  int32_t store_mode;
  int32_t ps_H, ps_W, ps_C; /* pixel-shuffle geometry: input grid H x W, Cout */
  du_conv_geom geom;  /* used by the IM2COL operand (at most one operand is IM2COL) */
  float* ws; int64_t ws_elems; /* optional scratch, du_gemm_ws_elems(args) floats (0 = none wanted for this product); without it the
                                  product still runs, on the plain tile kernels */
  const float* rope_sin; const float* rope_cos; int32_t rope_prefix; float rope_qscale;   /* DU_STORE_QKV_ROPE only */
  float* a_colsum;    /* optional, weight-gradient products only (a_mode PLAIN_COL, bf16): a_colsum[m] += sum_k A(m, k), fp32 atomics
                         into a buffer the caller zero-initialised -- the bias gradient sum_rows dY for free while dY^T X streams dY
                         anyway (nn.Linear backward).  du_gemm returns DU_ERR_UNSUPPORTED if the kernel family serving the product
                         cannot do it (du_gemm_route != 1 and != 5): call du_colsum then.  The side sum carries the product's `alpha`
                         (a_colsum[m] += alpha * sum_k A(m, k): the per-sample DropPath scale of the grouped jobs needs it); pass alpha = 1
                         for a plain bias gradient */
  float* b_colsum;    /* optional, ConvTranspose2d k2 s2 weight-gradient products only (a_mode PLAIN_COL, b_mode IM2COL_COL, bf16):
                         b_colsum[n % geom.C] += sum_k B(n, k) -- every dY pixel appears exactly once among the (input pixel, tap) pairs, so
                         this is the bias gradient sum_pixels dY[.., co]; same contract as a_colsum (zero-initialised, atomics,
                         DU_ERR_UNSUPPORTED unless du_gemm_route is 1 or 5) */
  float* C2;          /* DU_STORE_MSDA_PREP only: the second result (attention weights) */
  void* ks_ws;        /* optional scratch for workgroups that meet INSIDE a launch: the K-sliced ragged-row units of a tall product with a long
                         contraction (the ViT's fc2: M = 8 x 1029, K = 4096) and the K-split pair kernel (option key 16):
                         du_gemm_ks_ws_bytes(args) bytes that PERSIST between calls on one stream; the first 131072 bytes zeroed ONCE by
                         the caller (every launch leaves them zero again), the rest uninitialised.  One buffer per stream that may run
                         such products concurrently.  NULL / too small: one unit per 32 columns, one workgroup per tile */
  int64_t ks_ws_bytes;
} du_gemm_args;

int du_gemm(const du_gemm_args* args, void* stream);
/* Scratch du_gemm can use for `args` (ws / ws_elems are ignored here).  Non-zero for tall bf16 "NT" products whose row count
   leaves a short ragged last tile row on an otherwise exactly filled GPU (the ViT's M = 8 * 1029): those rows then go through a
   K-parallel skinny kernel pair instead of opening a nearly empty extra round of 128 x 128 tiles. */
int64_t du_gemm_ws_elems(const du_gemm_args* args);
/* Bytes of ks_ws du_gemm would use for `args` (0: nothing in this product meets inside the launch: shape, epilogue, du_set_option keys
   16 / 17). */
int64_t du_gemm_ks_ws_bytes(const du_gemm_args* args);
/* Kernel family du_gemm runs for the bulk of `args` AS PASSED (ws / ks_ws included: without ws the ragged rows stay in the tile grid and
   the choice is made for the whole M).  Read from the plan du_gemm executes (csrc/gemm_plan.h), so it is what runs: 0 generic (gemm.hip),
   1 bf16 tile engine (gemm_bf16.hip), 2 128 x 128 direct-to-LDS NT kernel (gemm_glds.hip), 3 / 4 the 256 x 256 / 256 x 128 multi-phase NT
   kernels (gemm_p8.hip), 5 the multi-phase weight-gradient kernel (gemm_p8.hip, TN form; also the 4-wave 256 x 128 NT kernel of
   du_set_option(0, 3)), 6 the persistent 256 x 128 kernel (gemm_p8.hip), 7 the resident-weights streaming kernel for K <= 256
   (gemm_rk.hip), 8 the 256 x 256 kernel as K-split pairs (gemm_p8.hip, option key 16).  Meaningless where du_gemm refuses `args`. */
int du_gemm_route(const du_gemm_args* args);
/* The whole plan du_gemm would execute for `args`, without launching (pure host logic: checkable without a GPU).  Writes 9 values and
   returns 9 (DU_ERR_BAD_ARG: NULL / n < 9): out[0] what du_gemm would return before any launch (DU_OK, DU_ERR_BAD_ARG, DU_ERR_UNSUPPORTED),
   [1] family (du_gemm_route), [2] variant: the multi-phase NT kernel 1 .. 5 (256 x 256, 256 x 128, 256 x 128 on 4 waves, persistent,
   K-split pairs), 0 for the other families, [3] 1 = the ConvTranspose2d k2 s2 operand is gathered from dY in place, [4] tail_rows: rows
   behind the last full tile row that leave the tile grid, [5] how: 0 none, 1 extra workgroups in the head's launch, 2 the one-launch
   skinny kernel, 3 the skinny partial + finish pair (through ws), 4 the bf16 tile engine, [6] K splits of family 5, [7] du_gemm_ws_elems,
   [8] du_gemm_ks_ws_bytes. */
int du_gemm_plan_describe(const du_gemm_args* args, int64_t* out, int n);

/* ---- grouped weight gradients: several dW = dY^T X products in ONE launch ----------------------------------------------------------
   The reference computes every weight gradient inside its layer's backward (torch autograd: F.linear / conv backward at
   dinov3_adapter.py:85-89,140-156, ms_deform_attn.py:158-216); nothing reads one before clip_grad_norm_ / optimizer.step()
   (nnUNetTrainer.py:919-928), so the host may queue them and launch them together.  Each job: C[m][n] (+)= sum_k A[k][m] * B[k][n] with
   A = dY (K rows, M columns, row stride lda), B = X (K rows, N columns, row stride ldb), bf16; C fp32 (M, N), row stride ldc, ZEROED by
   the caller (jobs that get more than one K split add into it atomically); a_colsum (nullable, zeroed, M floats): += sum_k A[k][m], the
   bias gradient.  The 256 workgroups of a launch are dealt out over the jobs in proportion to their contraction length.
   du_gemm_tn_group_legal: 1 if a job can be queued (K % 128 == 0, K >= 512, lda / ldb % 8 == 0, 16-byte aligned operands, < 2 GB
   operands); du_gemm_tn_group returns DU_ERR_UNSUPPORTED if any job is not.
   Convolution weight gradients (gather != 0) read B in place from an NHWC tensor, K = B * Hs * Ws contraction pixels (Ws -- and for
   gather 3 also Hs -- a power of two; gather 3: Ws % 64 == 0, a 64-pixel K-tile lies inside one image row), Cb channels per tap
   (Cb % 8 == 0), N = taps * Cb:
     gather 2: nn.ConvTranspose2d(k 2, s 2) (dinounet_training.py:255-264,558; dinov3_adapter.py:360): A = x (K, M = Cin), B(k, (tap, co)) =
               dy[pixel (2y + tap / 2, 2x + tap % 2)][co] with dy (B, 2 Hs, 2 Ws, Cb), pixel stride ldb; b_colsum (nullable, Cb floats,
               zeroed) += the bias gradient sum_pixels dy;
     gather 3: 3 x 3 / stride 1 / pad 1 convolution (the U-Net decoder blocks, dinounet_training.py:581-592): A = dy (K, M = Cout),
               B(k, (tap, ci)) = x[pixel + (tap / 3 - 1, tap % 3 - 1)][ci], zero outside the image; x (B, Hs, Ws, Cb), pixel stride ldb.
               A convolution over a fused channel concat (dinounet_training.py:614) is queued as one job per source.
   taps > 1: C is written in torch's weight layout, element (m, c_off + c, tap) at (m * inner_total + c_off + c) * taps + tap (inner = Cb
   channels in this job, inner_total in the parameter): the gradient of a (Cout, Cin, 3, 3) or (Cin, Cout, 2, 2) parameter without a
   permute afterwards; ldc is ignored. */
typedef struct du_tn_job {
  const void* A; int64_t lda;
  const void* B; int64_t ldb;
  float* C; int64_t ldc;
  float* a_colsum;
  const float* alpha;        /* nullable: scale of the whole product, read from device memory at run time (DropPath's per-sample scale in
                                backward, dinov3_adapter.py:18-37,148: the caller queues one job per sample); *alpha == 0 costs nothing */
  int32_t M, N, K;
  int32_t accumulate;        /* != 0: other jobs add into the same C / a_colsum (per-sample jobs, a parameter shared by several layers) */
  float* b_colsum;
  int32_t gather, Hs, Ws, Cb, taps, inner, inner_total, c_off;
} du_tn_job;
int du_gemm_tn_group_legal(const du_tn_job* job);
int du_gemm_tn_group(const du_tn_job* jobs, int njobs, void* stream);

/* ---- LDS-tiled direct 3x3 convolution (stride 1, pad 1), bf16 NHWC: decoder / FAPM / SPM-stem convs (dinounet_training.py:581-592,
        dinov3_adapter.py:243-249) and, with flipped + transposed weights, their data gradients --------------------------------------- */
/* Who decides: du_conv3x3_plan / du_conv3x3_wgrad_plan (csrc/conv_plan.h) choose the kernel, its instantiation, the rows of partial
   statistics and the number of partial dW slabs, once and before anything launches.  The entries below execute or read those plans, so
   what du_conv3x3_plan_describe / du_conv3x3_wgrad_plan_describe report for a call is what that call runs. */
/* x (B,H,W,C1) [+ x2 (B,H,W,Cin-C1): fused concat, nullable]; w bf16 [Cout][9*Cin] in (tap, ci) column order; y (B,H,W,Cout).
   stats_part (nullable): (stats_parts of the plan, Cout, 2) fp32 partial (sum, sum of squares) of the outputs, the partials of
   one image contiguous -- feed to du_strip_finalize(G = B).  Executes the plan: returns its rc -- DU_ERR_UNSUPPORTED for calls no kernel
   serves (H%8, W%16, Cout not in {32,64,128}, channel counts not multiples of 32, misaligned operands, ...): the caller then uses du_gemm's
   implicit-GEMM path -- and DU_ERR_UNSUPPORTED for a non-null stats_part where the plan's stats_parts is 0. */
int du_conv3x3_halo(const void* x, int64_t ldx, const void* x2, int64_t ldx2, int C1, int Cin, int Cout, int B, int H, int W,
                    const void* w, const float* bias, void* y, int64_t ldy, float* stats_part, void* stream);
/* The plan of that call (nothing is dereferenced or launched).  Fills out[0..3], returns 4 (DU_ERR_BAD_ARG: NULL / n < 4): [0] what
   du_conv3x3_halo would return before any launch (DU_OK, DU_ERR_BAD_ARG, DU_ERR_UNSUPPORTED), [1] kernel: 0 none, 1 conv3x3_strip_kernel,
   2 conv3x3_halo_kernel, [2] its instantiation: strip NP * 10 + NCO (11, 12, 21, 22), halo CK * 10 + TN (641, 321, 642, 322, 324),
   [3] stats_parts: rows of the partial-statistics array the kernel writes when want_stats != 0; 0 = the call emits no statistics (a
   strip shape whose byte sizes the strip kernel declines runs on the tile kernel without them). */
int du_conv3x3_plan_describe(const void* x, int64_t ldx, const void* x2, int64_t ldx2, int C1, int Cin, int Cout, int B, int H, int W,
                             const void* w, const void* y, int64_t ldy, int want_stats, int64_t* out, int n);
/* A reader of the same plan: stats_parts of the dense, 16-byte aligned call with statistics (pixel strides = channel counts, a second
   source exactly when C1 != Cin); 0 = not served.  Callers with strided or sliced tensors ask du_conv3x3_plan_describe. */
int du_conv3x3_halo_parts(int C1, int Cin, int Cout, int B, int H, int W);
/* The streaming kernel alone (Cin in {32, 64 (one tensor, or a 32 + 32 concat)}, Cout in {32, 64}, W % 128 == 0, H % 8 == 0: one wave per
   32-column strip, weights in registers / an LDS image, rows by LDS-DMA; csrc/conv_strip.hip).  Arguments as du_conv3x3_halo; runs the
   calls whose plan names kernel 1, DU_ERR_UNSUPPORTED for every other. */
int du_conv3x3_strip(const void* x, int64_t ldx, const void* x2, int64_t ldx2, int C1, int Cin, int Cout, int B, int H, int W,
                     const void* w, const float* bias, void* y, int64_t ldy, float* stats_part, void* stream);
/* Weight gradient of the same convolution, dw (Cout, 9*Cin) fp32 in (tap, ci) column order (OVERWRITTEN).  part: scratch of
   (blocks of the plan) * Cout * 9*Cin floats.  Executes the plan: DU_ERR_UNSUPPORTED = not served -> use du_gemm's IM2COL_COL path.
   with_db != 0: the bias gradient db[co] = sum_pixels dy rides along -- dw then has Cout * 9*Cin + Cout elements (db behind the weight
   gradient) and part blocks * (Cout * 9*Cin + Cout). */
int du_conv3x3_wgrad_halo(const void* x, int64_t ldx, const void* x2, int64_t ldx2, int C1, int Cin, int Cout, int B, int H, int W,
                          const void* dy, int64_t lddy, float* part, float* dw, int with_db, void* stream);
/* The plan of that call.  Fills out[0..3], returns 4 (DU_ERR_BAD_ARG: NULL / n < 4): [0] rc as above, [1] kernel: 0 none,
   1 conv3x3_wgrad_rows_kernel, 2 the round-3 conv3x3_wgrad_halo_kernel (du_set_option key 13 = 0, or a tensor past the rows kernel's 32-bit
   offsets, judged on the strides passed), [2] its instantiation CK * 10 + MT, [3] blocks: workgroups = partial dW slabs, keyed on [1]. */
int du_conv3x3_wgrad_plan_describe(const void* x, int64_t ldx, const void* x2, int64_t ldx2, int C1, int Cin, int Cout, int B, int H, int W,
                                   const void* dy, int64_t lddy, int64_t* out, int n);
/* A reader of the same plan: blocks of the dense, 16-byte aligned call (as du_conv3x3_halo_parts); 0 = not served. */
int du_conv3x3_wgrad_halo_blocks(int C1, int Cin, int Cout, int B, int H, int W);
/* out[g][c][j] = sum_s part[g*strips + s][c][j]: second stage of the column reductions, exposed for producers that emit partials */
int du_strip_finalize(const float* part, float* out, int G, int strips, int C, void* stream);

/* ---- ViT attention -------------------------------------------------------------------------- */
/* qkv: (B, N, 3, H, Dh) as produced by the fused QKV GEMM.  Writes q (scaled by `qscale`), k, v as
   (B, H, Npad, Dh) (rows >= N untouched: the caller zero-fills once); RoPE (rotate-half form, fp32 math) is
   applied to q and k for tokens >= prefix using sin/cos tables (N - prefix, Dh) fp32. */
int du_qkv_rope_split(int dtype, const void* qkv, void* q, void* k, void* v, const float* sin_t, const float* cos_t,
                      int B, int N, int Npad, int H, int Dh, int prefix, float qscale, void* stream);
/* The same for the token rows [m_begin, m_begin + m_count) of the (B * N, 3 * H * Dh) matrix only; qkv_rows points at row m_begin (the
   rows a tile kernel left to the skinny tail when it wrote the rest through DU_STORE_QKV_ROPE). */
int du_qkv_rope_split_rows(int dtype, const void* qkv_rows, void* q, void* k, void* v, const float* sin_t, const float* cos_t, int B, int N,
                           int Npad, int H, int Dh, int prefix, float qscale, int64_t m_begin, int m_count, void* stream);
/* RoPE + q scale IN PLACE on head-major q / k planes (B, H, Npad, Dh) that du_gemm stored unrotated (DU_STORE_QKV_HEADS): the arithmetic of
   du_qkv_rope_split on rows b * N + n < m_limit (rows at and behind m_limit were written, rotated, by du_qkv_rope_split_rows); bf16.
   Replaces layers/attention.py:66-85 like du_qkv_rope_split. */
int du_qkv_rope_inplace(int dtype, void* q, void* k, const float* sin_t, const float* cos_t, int B, int N, int Npad, int H, int Dh,
                        int prefix, float qscale, int64_t m_limit, void* stream);
/* Non-causal softmax2(q k^T) v per (b, head) with base-2 exponentials: q must be pre-scaled by
   Dh^-0.5 * log2(e).  q,k,v: (B, H, Npad, Dh) bf16; out: (B, N, H*Dh) bf16.  Dh in {64, 128}. */
int du_attention_fwd(const void* q, const void* k, const void* v, void* out, int B, int H, int N, int Npad, int Dh,
                     void* stream);
/* row softmax over the first `cols` entries of each row of a (rows, ld) fp32 matrix, in place; entries
   [cols, ld) are zeroed (parity-mode attention with materialised scores). */
int du_softmax_rows_f32(float* x, int64_t rows, int cols, int64_t ld, void* stream);

/* ---- LayerNorm -------------------------------------------------------------------------------- */
int du_layernorm_fwd(int in_dtype, int out_dtype, const void* x, int64_t ldx, const float* w, const float* b, void* y,
                     int64_t ldy, float* mean_out, float* rstd_out, int64_t rows, int D, float eps, void* stream);
/* Column reductions (statistics, bias / norm-parameter gradients) run in two stages when the caller lends a scratch buffer
   `ws` of at least du_reduce_ws_elems(...) floats: every workgroup writes its strip's partial sums, a second kernel adds them
   up and OVERWRITES the result buffer.  With ws == NULL the partials are accumulated with fp32 atomics into a result buffer the
   caller must have zero-filled (same-cache-line atomics serialise: ~0.1 us each, measured, so this is the slow fallback). */
int64_t du_reduce_ws_elems(int dtype, int G, int64_t pix_per_group, int C);
/* dx (same dtype as x); dwdb fp32: with scratch (du_reduce_ws_elems(dtype, 1, rows, D) floats) PLANAR dw[D] then db[D]; with ws == NULL the
   atomics fallback accumulates (dw[c], db[c]) interleaved into a zero-filled (D, 2) buffer.
   dres (nullable, same dtype/shape as x): gradient of a residual branch that by-passes the norm, added into dx. */
int du_layernorm_bwd(int dtype, const void* x, const void* dy, const float* w, const float* mean, const float* rstd,
                     void* dx, float* dwdb, int64_t rows, int D, float* ws, int64_t ws_elems, const void* dres, void* stream);
/* du_layernorm_bwd whose dy is a narrow product that is never written: dy = bf16(G Wt^T) with fp32 accumulation and one rounding -- G
   (rows, K) bf16 with row stride ldg, Wt (D, K) bf16 with row stride ldw (the K-contiguous operand of the unfused data gradient) -- then the
   arithmetic of du_layernorm_bwd on dense (rows, D) x / dx / dres (csrc/norm_gemm.hip: a workgroup owns whole rows and keeps their dy in
   LDS).  dwdb: PLANAR dw[D] then db[D]; the scratch is required, out[4] of the plan in floats.
   The library decides once per call (csrc/norm_gemm_plan.h): bf16, D == 1024, K % 64 == 0 and K <= 256, ldg / ldw multiples of 8 and >= K,
   x / G / Wt / dx / dres 16-byte aligned; every other call is DU_ERR_UNSUPPORTED before anything launches and the caller runs the data
   gradient and du_layernorm_bwd.  _plan reads the same decision from the call's numbers alone (no operand is dereferenced):
   out[0..5] = {served (1 / 0), rows per block, workgroups, rows per workgroup, scratch floats, LDS bytes}; returns 6, DU_ERR_BAD_ARG for
   out == NULL or n < 6. */
int du_layernorm_bwd_prod_plan(int dtype, const void* x, const void* G, int64_t ldg, const void* Wt, int64_t ldw, int K, const void* dx,
                               const void* dres, int64_t rows, int D, int64_t* out, int n);
int du_layernorm_bwd_prod(int dtype, const void* x, const void* G, int64_t ldg, const void* Wt, int64_t ldw, int K, const float* w,
                          const float* mean, const float* rstd, void* dx, float* dwdb, int64_t rows, int D, float* ws, int64_t ws_elems,
                          const void* dres, void* stream);

/* ---- channel-statistics norms (InstanceNorm2d / BatchNorm2d over NHWC) ---------------------------- */
/* sums[g][c][0..1] += (sum x, sum x^2) over the pixels of group g (G groups of `pix_per_group` pixels). */
int du_chan_stats(int dtype, const void* x, int64_t ldx, float* sums, int G, int64_t pix_per_group, int C, float* ws,
                  int64_t ws_elems, void* stream);
/* out[c] = sum over rows of x[row][c] (bias gradients); scratch of du_reduce_ws_elems(dtype, 1, rows, C) floats is required */
int du_colsum(int dtype, const void* x, int64_t ldx, float* out, int64_t rows, int C, float* ws, int64_t ws_elems, void* stream);
/* sums[g][c][0..1] += (sum a*b, sum a) over the pixels of group g (squeeze-excitation gate gradient, a = dy, b = x). */
int du_chan_dot(int dtype, const void* a, int64_t lda, const void* b, int64_t ldb, float* sums, int G, int64_t pix_per_group, int C,
                float* ws, int64_t ws_elems, void* stream);
/* mean = sum/count, rstd = rsqrt(max(sumsq/count - mean^2, 0) + eps) for sums (G,C,2) -> (G,C); with run_mean/run_var (nullable, G = 1):
   BatchNorm running-statistics update, momentum m, unbiased variance (torch semantics). */
int du_norm_stats_finalize(const float* sums, float count, float eps, float* mean, float* rstd, int G, int C, float* run_mean,
                           float* run_var, float momentum, void* stream);
/* affine-parameter gradients from the backward sums: dw[c] = sum_g bsums[g][c][1], db[c] = sum_g bsums[g][c][0] */
int du_norm_param_grads(const float* bsums, float* dw, float* db, int G, int C, void* stream);
/* Fused forms (one launch less each: a launch of this size costs ~5 us inside the replayed graph).  All three need the scratch of
   du_reduce_ws_elems (no atomics fallback):
   du_chan_stats_norm       = du_chan_stats + du_norm_stats_finalize (sums nullable);
   du_strip_finalize_norm   = du_strip_finalize + du_norm_stats_finalize, for statistics partials from a convolution epilogue;
   du_norm_act_bwd_stats_grads = du_norm_act_bwd_stats + du_norm_param_grads (bsums, dw, db all written). */
int du_chan_stats_norm(int dtype, const void* x, int64_t ldx, float* sums, int G, int64_t pix_per_group, int C, float* ws, int64_t ws_elems,
                       float count, float eps, float* mean, float* rstd, float* run_mean, float* run_var, float momentum, void* stream);
int du_strip_finalize_norm(const float* part, float* sums, int G, int strips, int C, float count, float eps, float* mean, float* rstd,
                           float* run_mean, float* run_var, float momentum, void* stream);
int du_norm_act_bwd_stats_grads(int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, const float* mean, const float* rstd,
                                const float* w, const float* b, float* bsums, float* dw, float* db, int G, int64_t pix_per_group, int C,
                                int act, float* ws, int64_t ws_elems, void* stream);
/* y = act((x - mean[g,c]) * rstd[g,c] * w[c] + b[c]); mean/rstd: (G, C) fp32. */
int du_norm_act_fwd(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, const float* mean, const float* rstd,
                    const float* w, const float* b, int G, int64_t pix_per_group, int C, int act, void* stream);
/* backward pass 1: through the activation, accumulate per-(g,c) sum(dz) and sum(dz*xhat) into bsums (G,C,2). */
int du_norm_act_bwd_stats(int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, const float* mean,
                          const float* rstd, const float* w, const float* b, float* bsums, int G, int64_t pix_per_group,
                          int C, int act, float* ws, int64_t ws_elems, void* stream);
/* backward pass 2: dx = w*rstd*(dz - s1/n - xhat*s2/n) with (s1,s2) from bsums (G,C,2) and n = `count` (pixels the
   statistics were taken over: pix_per_group for IN, all pixels x world for BN).  use_batch_stats=0 => dx = dz*w*rstd */
int du_norm_act_bwd_dx(int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, void* dx, int64_t lddx,
                       const float* mean, const float* rstd, const float* w, const float* b, const float* bsums, int G,
                       int64_t pix_per_group, int C, int act, float count, int use_batch_stats, void* stream);

/* ---- multi-scale deformable attention ---------------------------------------------------------------- */
/* value (N, S, M, D); spatial_shapes (L,2) int64 (H,W); level_start_index (L) int64; sampling_loc (N,Lq,M,L,P,2)
   as (x,y) in [0,1]; attn_weight (N,Lq,M,L,P); out (N,Lq,M*D).  value/out dtype = `dtype`; loc/weights fp32 when
   dtype is BF16, same as value when F32.  Semantics: ms_deform_im2col_cuda.cuh:242-304. */
int du_msda_forward(int dtype, const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                    const float* sampling_loc, const float* attn_weight, void* out, int N, int S, int M, int D, int L,
                    int Lq, int P, void* stream);
/* grad_value (fp32, N,S,M,D), grad_sampling_loc, grad_attn_weight (fp32): OVERWRITTEN -- the caller need not zero them (the
   reference allocates them with at::zeros, ms_deform_attn_cuda.cu:126-128; here the library clears grad_value itself on the
   paths that scatter into it atomically and writes every element of the other two). */
/* Optional scratch `ws` (du_msda_bwd_ws_elems floats, 0 = not needed for this shape): the LDS-resident kernel then writes one
   partial grad_value plane per query chunk with plain stores and a second kernel sums them into grad_value (OVERWRITING it)
   instead of flushing every chunk with global fp32 atomics. */
int64_t du_msda_bwd_ws_elems(int N, int S, int M, int D, int L, int Lq, int P);
int du_msda_backward(int dtype, const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                     const float* sampling_loc, const float* attn_weight, const void* grad_out, float* grad_value,
                     float* grad_sampling_loc, float* grad_attn_weight, int N, int S, int M, int D, int L, int Lq, int P,
                     float* ws, int64_t ws_elems, void* stream);

/* fp64 forms: the reference extension dispatches AT_DISPATCH_FLOATING_TYPES (fp32 and fp64, ops/src/cuda/ms_deform_attn_cuda.cu:69,139) and
   its acceptance script feeds .double() tensors through MSDeformAttnFunction and torch.autograd.gradcheck (ops/test.py:40-58,101-121).
   Every tensor double (value, sampling_loc, attn_weight, out / the three gradients); same semantics; grad_value is cleared by the library. */
int du_msda_forward_f64(const double* value, const int64_t* spatial_shapes, const int64_t* level_start_index, const double* sampling_loc,
                        const double* attn_weight, double* out, int N, int S, int M, int D, int L, int Lq, int P, void* stream);
int du_msda_backward_f64(const double* value, const int64_t* spatial_shapes, const int64_t* level_start_index, const double* sampling_loc,
                         const double* attn_weight, const double* grad_out, double* grad_value, double* grad_sampling_loc,
                         double* grad_attn_weight, int N, int S, int M, int D, int L, int Lq, int P, void* stream);

/* The same with grad_value written in bf16 (value's dtype: what the value projection's backward reads) -- no cast pass afterwards.
   bf16, one level, 4 points, D <= 32 only (the MFMA grad_value path); DU_ERR_UNSUPPORTED otherwise: use du_msda_backward and cast. */
int du_msda_backward_bf16gv(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index, const float* sampling_loc,
                            const float* attn_weight, const void* grad_out, void* grad_value_bf16, float* grad_sampling_loc,
                            float* grad_attn_weight, int N, int S, int M, int D, int L, int Lq, int P, float* ws, int64_t ws_elems,
                            void* stream);

/* MSDeformAttn glue (ms_deform_attn.py:188-197, single level): raw (rows, M*P*2 + M*P) = [offsets | logits] from the
   fused sampling_offsets/attention_weights GEMM; ref (Lq, 2) reference points (x, y);
   loc (rows, M, P, 2) = ref + off / (Ws, Hs); attn (rows, M, P) = softmax over P. */
int du_msda_prep(int dtype, const void* raw, int64_t ldr, const float* ref, float* loc, float* attn, int64_t rows, int Lq,
                 int M, int P, int Hs, int Ws, void* stream);
int du_msda_prep_bwd(int dtype, const float* attn, const float* gloc, const float* gattn, void* graw, int64_t ldr,
                     int64_t rows, int M, int P, int Hs, int Ws, void* stream);

/* ---- small conv-side ops (NHWC; `*bs` = per-image stride in elements so token ranges can be viewed as images) ---- */
/* Depthwise 3x3 (stride 1, pad 1), y = act(dwconv3x3(x) + bias); w: (C,3,3) fp32, bias (C, nullable) fp32.
   pyramid == 0: one NHWC segment, B images of H x W pixels; `ld` = pixel stride and `bs` = image stride in elements, shared by EVERY
   tensor of the call (x, y, z, dy, dx, dz: a call serves tensors laid out alike).
   pyramid != 0: ConvFFN's token pyramid (DWConv.forward, dinov3_adapter.py:99-109): contiguous (B, 21 n, C) token tensors, n = H*W/4, each
   image holding a (2H x 2W), an (H x W) and an (H/2 x W/2) grid back to back, one launch per pass; ld == C and bs == 21 n C.
   The library picks the kernel (csrc/dwconv_plan.h: du_dwconv_plan decides once per call, the entries below execute or read it): the
   band kernels of dwconv.hip for bf16, C % 8 == 0, even grid widths, ld % 8 == 0, bs % 8 == 0 -- the pyramid with any activation, an
   NHWC segment with DU_ACT_NONE -- and the row kernels of elementwise.hip otherwise (C, ld, bs multiples of 8 bf16 / 4 fp32; H, W even
   for the pyramid).  y, z and dx have the same bits on either family; dw / db are the same fp32 sums in another order.
   _fwd: z (nullable) receives the pre-activation, which the backward of `act` needs.
   _bwd: ONE call per backward; it OVERWRITES dx, dw (C,9) and db (C, nullable) and needs du_dwconv3x3_bwd_ws_elems floats of scratch
   (partial rows, summed by a small second launch; fewer is DU_ERR_BAD_ARG before anything launches).  z (pre-activation) and dz (scratch,
   shaped as dy) are required exactly when act != DU_ACT_NONE: dz = dy * act'(z) is formed on load by the band data gradient, by a launch
   of du_act_bwd's kernel in the row family -- which needs dense tensors (ld == C, bs == H*W*C) there: DU_ERR_UNSUPPORTED otherwise.
   _plan_describe: out[0..6] = {rc the call would return before launching, forward / data-gradient kernel (1 dwconv_kernel, 2
   dwconv_row4_kernel, 3 dwconv_band_kernel), its band height (0: row kernels), activation backward (0 none, 1 a separate act_bwd_kernel
   launch, 2 on load in dwconv_band_dgrad_act_kernel), weight-gradient kernel (1 dwconv_bwd_weight_kernel<T, false>, 2 <T, true>,
   3 <bf16, true, true>, 4 dwconv_band_wgrad_kernel), its partial rows, scratch floats}; returns 7, DU_ERR_BAD_ARG for out == NULL or n < 7. */
int du_dwconv3x3_fwd(int dtype, const void* x, const float* w, const float* bias, void* y, void* z, int64_t ld, int64_t bs, int B, int H,
                     int W, int C, int pyramid, int act, void* stream);
int64_t du_dwconv3x3_bwd_ws_elems(int dtype, int64_t ld, int64_t bs, int B, int H, int W, int C, int pyramid, int act);
int du_dwconv3x3_bwd(int dtype, const void* z, const void* dy, const void* x, const float* w, void* dx, float* dw, float* db, void* dz,
                     int64_t ld, int64_t bs, int B, int H, int W, int C, int pyramid, int act, float* ws, int64_t ws_elems, void* stream);
int du_dwconv3x3_plan_describe(int dtype, int64_t ld, int64_t bs, int B, int H, int W, int C, int pyramid, int act, int64_t* out, int n);
/* MaxPool2d(3, 2, 1) on contiguous NHWC; idx (nullable, same shape as y, uint8) records the winning tap */
int du_maxpool3x3s2_fwd(int dtype, const void* x, void* y, uint8_t* idx, int B, int H, int W, int C, void* stream);
int du_maxpool3x3s2_bwd(int dtype, const uint8_t* idx, const void* dy, void* dx, int B, int H, int W, int C, void* stream);
/* out = base + bilinear_upsample(src) (align_corners=False); src (B,Hs,Ws,C) of src_dtype, base/out (B,Ho,Wo,C).  base == NULL: the
   plain resize F.interpolate(src, size=(Ho,Wo), mode='bilinear', align_corners=False) (tail of LearnableUpsampleBlock,
   dinounet_training.py:262-263) */
int du_bilinear_add_fwd(int src_dtype, int dtype, const void* src, int64_t lds_, const void* base, int64_t ldb, void* out,
                        int64_t ldo, int B, int Hs, int Ws, int Ho, int Wo, int C, void* stream);
/* data gradient of that resize: dx (B,Hs,Ws,C) from dy (B,Ho,Wo,C); gather form (deterministic, no atomics) */
int du_bilinear_resize_bwd(int dtype, const void* dy, int64_t lddy, void* dx, int64_t lddx, int B, int Hs, int Ws, int Ho, int Wo,
                           int C, void* stream);
/* dz = dy * act'(z) */
int du_act_bwd(int dtype, const void* z, const void* dy, void* dz, int64_t n, int act, void* stream);

/* ---- squeeze-excitation (SqueezeExcitation, dinounet_training.py:210-225; residual add of :438 fused) -------------- */
/* sums (B,C,2) from du_chan_stats(G=B); W1 (R,C), b1 (R), W2 (C,R), b2 (C) fp32; hidden (B,R) post-ReLU, gate (B,C) = sigmoid. */
int du_se_gate_fwd(const float* sums, float inv_count, const float* W1, const float* b1, const float* W2, const float* b2,
                   float* hidden, float* gate, int B, int C, int R, void* stream);
/* y = x * gate[b][c] (+ shortcut, nullable) over (B, P pixels, C) NHWC */
int du_se_scale_fwd(int dtype, const void* x, int64_t ldx, const float* gate, const void* shortcut, int64_t ldsc, void* y, int64_t ldy,
                    int B, int64_t P, int C, void* stream);
/* dsum (B,C,2) from du_chan_dot(dy, x).  Writes dpool (B,C) (gradient reaching every pixel through the pooling path, already
   divided by P) and the gate-MLP parameter gradients dW1 (R,C), db1 (R), dW2 (C,R), db2 (C). */
int du_se_gate_bwd(const float* dsum, const float* sums, float inv_count, const float* gate, const float* hidden, const float* W1,
                   const float* W2, float* dpool, float* dW1, float* db1, float* dW2, float* db2, int B, int C, int R, void* stream);
/* dx = dy * gate[b][c] + dpool[b][c] */
int du_se_scale_bwd(int dtype, const void* dy, int64_t lddy, const float* gate, const float* dpool, void* dx, int64_t lddx, int B,
                    int64_t P, int C, void* stream);

/* ---- trainer loss: DC_and_CE_loss (training/loss/compound_losses.py:8-56, dice.py:58-119: batch dice, no background, smooth 1e-5) ---- */
/* logits (B,K,H,W) fp32 NCHW, target (B,H*W) int64 labels, K in [2,8] (K < 2: DU_ERR_BAD_ARG, K > 8:
   DU_ERR_UNSUPPORTED, before any launch).  sums: 1 + 3(K-1) floats = [sum -log p_t, (I_c, P_c, G_c) c>=1].
   scratch: du_dice_ce_ws_elems floats (0 for a K outside [2,8]).  Under data parallelism the caller all-reduces sums[1:] between _sums and _finish. */
int64_t du_dice_ce_ws_elems(int B, int K, int64_t HW);
int du_dice_ce_sums(const float* logits, const int64_t* target, float* sums, int B, int K, int64_t HW, float* ws, int64_t ws_elems,
                    void* stream);
/* loss (1 float) = CE - mean_c dice_c; coef (2(K-1)) = backward coefficients; npix = this rank's pixel count; grad_mult = world size
   when the dice sums were all-reduced, else 1 */
int du_dice_ce_finish(const float* sums, float* loss, float* coef, int K, int64_t npix, float smooth, float grad_mult, void* stream);
/* dlogits (B,K,H,W) fp32 = grad_out[0] * d loss / d logits (grad_out: device scalar or NULL for 1) */
int du_dice_ce_bwd(const float* logits, const int64_t* target, const float* coef, const float* grad_out, float* dlogits, int B, int K,
                   int64_t HW, void* stream);

/* ---- trainer loss with an ignore label: DC_and_CE_loss(ignore_label) (training/loss/compound_losses.py:31-56, dice.py:72-119 with
        loss_mask; nnUNetTrainer._build_loss, nnUNetTrainer.py:363-365) ---- */
/* logits (B,K,H,W) fp32, target (B,H*W) int64 in [0,K) or ignore_label, K in [2,8] (DU_ERR_UNSUPPORTED otherwise).  m = [t != ignore].
   sums: 2 + 3(K-1) floats = [sum m (-log p_t), n_valid, (I_c, P_c, G_c) c = 1..K-1], every term multiplied by m.  scratch:
   du_dice_ce_masked_ws_elems floats.  Under data parallelism the caller all-reduces sums[2:] only (CE and n_valid stay local). */
int64_t du_dice_ce_masked_ws_elems(int B, int K, int64_t HW);
int du_dice_ce_masked_sums(const float* logits, const int64_t* target, float* sums, int B, int K, int64_t HW, int64_t ignore_label,
                           float* ws, int64_t ws_elems, void* stream);
/* loss (1 float) = CE_sum * ce_scale - mean_c dice_c with ce_scale = 1/n_valid, or 0 when n_valid = 0 (compound_losses.py:52-53, decided
   on the device); coef (2(K-1) + 1) = dice backward coefficients then ce_scale; grad_mult = world size when sums[2:] were all-reduced */
int du_dice_ce_masked_finish(const float* sums, float* loss, float* coef, int K, float smooth, float grad_mult, void* stream);
/* dlogits = grad_out[0] * d loss / d logits; exactly 0 in every channel of an ignored pixel */
int du_dice_ce_masked_bwd(const float* logits, const int64_t* target, const float* coef, const float* grad_out, float* dlogits, int B,
                          int K, int64_t HW, int64_t ignore_label, void* stream);

/* ---- top-k losses: TopKLoss (training/loss/robust_ce_loss.py:19-32) and DC_and_topk_loss (compound_losses.py:102-150) ---- */
/* logits (B,K,H,W) fp32, target (B,H*W) int64 in [0,K) or, with has_ignore, ignore_label; K in [2,8] (DU_ERR_UNSUPPORTED otherwise),
   N = B H W < 2^31, 1 <= k_vox <= N (DU_ERR_BAD_ARG otherwise, before any launch).  v = -log p_t per voxel, +0 where ignored.
   du_topk_loss_fwd: values (N fp32) = v; sums (2 + 3(K-1) floats) = [sum v, n_valid, (I_c, P_c, G_c) c = 1..K-1], the masked loss's
   layout (under data parallelism the caller all-reduces sums[2:] only; the top-k is local); the radix select of the k_vox-th largest v
   and the per-wave sums above it are left in ws (du_topk_loss_ws_elems 4-byte words, 16-byte aligned), which du_topk_loss_finish reads:
   loss (1 float) = mean of the k_vox largest v, minus mean_c dice_c when dice != 0; coef (2(K-1) + 1) = the Dice backward
   coefficients (zeros when dice == 0) then 1 / k_vox; sel (N uint8) = 1 on exactly k_vox voxels: every v > T and, among v == T, the
   lowest flat indices; info (4 int32) = (bits of T, k_vox - #{v > T}, #{v > T}, 0); grad_mult = world size when sums[2:] were
   all-reduced.  du_topk_loss_bwd: dlogits = grad_out[0] * d loss / d logits with the selection read from sel; exactly 0 in every
   channel of an ignored voxel.  No float atomics: bit-reproducible. */
int64_t du_topk_loss_ws_elems(int B, int K, int64_t HW);
int du_topk_loss_fwd(const float* logits, const int64_t* target, float* values, float* sums, int B, int K, int64_t HW, int has_ignore,
                     int64_t ignore_label, int64_t k_vox, int32_t* ws, int64_t ws_elems, void* stream);
int du_topk_loss_finish(const float* sums, const float* values, int32_t* ws, int64_t ws_elems, uint8_t* sel, float* loss, float* coef,
                        int32_t* info, int B, int K, int64_t HW, int64_t k_vox, int dice, float smooth, float grad_mult, void* stream);
int du_topk_loss_bwd(const float* logits, const int64_t* target, const uint8_t* sel, const float* coef, const float* grad_out,
                     float* dlogits, int B, int K, int64_t HW, int has_ignore, int64_t ignore_label, void* stream);

/* ---- trainer loss for regions: DC_and_BCE_loss (training/loss/compound_losses.py:59-99; MemoryEfficientSoftDiceLoss with sigmoid,
        do_bg=True, dice.py:58-119; nnUNetTrainer.py:356-361) ---- */
/* logits (B,R,H,W) fp32, target (B,R+has_ignore,H*W) uint8 in {0,1}, R in [1,8] (DU_ERR_UNSUPPORTED otherwise).  With has_ignore the last
   target plane is the ignore channel and m = 1 - target[:, R], else m = 1.  sums: 2 + 3R floats = [sum m bce, n_valid (pixels),
   (I_r, P_r, G_r) r = 0..R-1].  Under data parallelism the caller all-reduces sums[2:] only. */
int64_t du_dice_bce_ws_elems(int B, int R, int64_t HW);
int du_dice_bce_sums(const float* logits, const uint8_t* target, float* sums, int B, int R, int64_t HW, int has_ignore, float* ws,
                     int64_t ws_elems, void* stream);
/* loss (1 float) = BCE_sum * bce_scale - mean_r dice_r, bce_scale = 1/n_valid with has_ignore (compound_losses.py:95: the mask is
   (B,1,H,W), the denominator counts pixels), else 1/(n_valid R) (the mean over every element), 0 when n_valid = 0; coef (2R + 1) */
int du_dice_bce_finish(const float* sums, float* loss, float* coef, int R, int has_ignore, float smooth, float grad_mult, void* stream);
int du_dice_bce_bwd(const float* logits, const uint8_t* target, const float* coef, const float* grad_out, float* dlogits, int B, int R,
                    int64_t HW, int has_ignore, void* stream);
/* ConvertSegmentationToRegionsTransform (data_augmentation/custom_transforms/region_based_training.py:7-37, nnUNetTrainer.py:764-767):
   seg (B,H*W) int64, table (R) int64 DEVICE bit masks (bit l set = label l belongs to region r; labels 0..63, any other label is in no
   region), out (B,R+has_ignore,H*W) uint8: plane r = [seg in region r], plane R = [seg == ignore_label] */
int du_labels_to_regions(const int64_t* seg, const int64_t* table, uint8_t* out, int B, int R, int64_t HW, int has_ignore,
                         int64_t ignore_label, void* stream);

/* ---- the trainer losses with the options of the reference's loss classes (csrc/loss_opt.hip): weight_ce / weight_dice
        (compound_losses.py:8-99), batch_dice / do_bg (MemoryEfficientSoftDiceLoss, dice.py:58-119), class weights of the CE
        (RobustCrossEntropyLoss = nn.CrossEntropyLoss(weight)).  The defaults keep the entry points above. ---- */
typedef struct {
  int n;               /* K classes in [2,8] (softmax) or R regions in [1,8] (DU_ERR_UNSUPPORTED otherwise) */
  int regions;         /* 0: softmax, target (B,H*W) int64 labels; 1: sigmoid, target (B,R+has_ignore,H*W) uint8, ignore plane last */
  int has_ignore;      /* 0 / 1 */
  int64_t ignore;      /* the ignore label of a softmax target (read with has_ignore) */
  int do_bg;           /* softmax: class 0 has a Dice term; regions: must be 1 */
  int batch_dice;      /* 1: Dice sums over the batch (one row); 0: one row per image, the mean runs over (B, classes) */
  float weight_ce;     /* >= 0, finite, not both 0; a weight of 0 removes the term from the loss and from the gradient */
  float weight_dice;
  const float* class_w; /* DEVICE, n floats > 0, or NULL; softmax only: CE = sum w_t nll / sum w_t over the valid pixels */
} du_loss_opt;
/* A contradiction in `o` (a flag outside 0 / 1, a negative or non-finite weight, both weights 0, class_w or do_bg = 0 with regions), a
   null pointer or B, HW <= 0: DU_ERR_BAD_ARG before any launch.  CD = Dice classes = n - 1, n with do_bg, n for regions; rows = 1 with
   batch_dice, else B.  sums: (rows, 2 + 3 CD) floats = per row [sum w_t nll or sum m bce, sum w_t or n_valid, (I_c, P_c, G_c) c < CD];
   with rows = B the CE columns of the rows are added in the finish.  scratch: du_loss_opt_ws_elems floats (0: unsupported).  Under data
   parallelism the caller all-reduces sums[2:] of a batch_dice row and nothing otherwise.  du_loss_opt_finish: loss (1 float) =
   weight_ce CE - weight_dice mean Dice; coef (rows 2 CD + 1 floats) = [rows][(ca_c, cb_c) c < CD] with weight_dice / (CD rows) and
   grad_mult folded in, then weight_ce times the CE scale (0 when nothing is valid); a weight of 0 gives exact zeros.
   du_loss_opt_bwd: dlogits = grad_out[0] * d loss / d logits, exactly 0 in every channel of an ignored pixel.  Two-stage sums in an
   order that depends on the shape only, no float atomics: bit-reproducible. */
int64_t du_loss_opt_ws_elems(const du_loss_opt* o, int B, int64_t HW);
int du_loss_opt_sums(const du_loss_opt* o, const float* logits, const void* target, float* sums, int B, int64_t HW, float* ws,
                     int64_t ws_elems, void* stream);
int du_loss_opt_finish(const du_loss_opt* o, const float* sums, float* loss, float* coef, int B, float smooth, float grad_mult,
                       void* stream);
int du_loss_opt_bwd(const du_loss_opt* o, const float* logits, const void* target, const float* coef, const float* grad_out,
                    float* dlogits, int B, int64_t HW, void* stream);

/* ---- deep supervision: DeepSupervisionWrapper (training/loss/deep_supervision.py) around the three losses above, with the targets of
        DownsampleSegForDSTransform2 (custom_transforms/deep_supervision_donwsampling.py) gathered in the kernels ----
   total = sum over the scales with weights[s] != 0, in scale order, of weights[s] * loss_s.  logits / dlogits: HOST arrays of S DEVICE
   pointers, scale s = (B, C, hs[s], wd[s]) fp32, largest first; hs, wd, weights: HOST arrays of S values, read during the call.  A scale
   with weight 0 is inactive: its pointer may be NULL, its logits are never read and its gradient is never written.  target (B, H*W)
   int64: the FULL-resolution label map; the target of scale s at (y, x) is target[src(y, H / hs[s], H), src(x, W / wd[s], W)],
   src(i, z, n) = floor(clamp((i + 0.5) z - 0.5, 0, n - 1) + 0.5) in fp64, operation by operation what scipy.ndimage.zoom(order=0,
   mode="nearest", grid_mode=True) computes, i.e. batchgenerators' resize_segmentation(order=0).
   mode 0: softmax over C = K classes in [2,8], labels in [0,K) or ignore_label (has_ignore), Dice over classes 1..K-1 (CD = K-1);
   mode 1: sigmoid over C = R regions in [1,8], table (R) int64 DEVICE bit masks as in du_labels_to_regions, Dice over all R (CD = R).
   sums (S (2 + 3 CD) floats): [(CE or BCE sum, n_valid) per scale | (I_c, P_c, G_c) c < CD per scale]; under data parallelism the caller
   all-reduces sums[2 S:] (every scale's Dice slice, contiguous) and passes grad_mult = world size.  Zeros for an inactive scale.
   loss (1 + S floats) = [total, loss_0 .. loss_{S-1}] (0 for an inactive scale); coef (S (2 CD + 1) floats), weights folded in.
   Launches: du_ds_loss_sums 2 (partial rows of all scales; one block per scale adds its rows in a fixed order: no float atomics),
   du_ds_loss_finish 1, du_ds_loss_bwd 1 -- four per loss whatever S is.
   DU_ERR_BAD_ARG: S < 1, a scale larger than the target, a NULL pointer of an active scale, every weight 0, a workspace below
   du_ds_loss_ws_elems floats; DU_ERR_UNSUPPORTED: S > 4, C outside the ranges above, H or W above 32768. */
int64_t du_ds_loss_ws_elems(int mode, int B, int C, int H, int W, int S, const int* hs, const int* wd, const float* weights);
int du_ds_loss_sums(int mode, const float* const* logits, const int64_t* target, const int64_t* table, float* sums, int B, int C, int H,
                    int W, int S, const int* hs, const int* wd, const float* weights, int has_ignore, int64_t ignore_label, float* ws,
                    int64_t ws_elems, void* stream);
int du_ds_loss_finish(int mode, const float* sums, float* loss, float* coef, int C, int S, const float* weights, int has_ignore,
                      float smooth, float grad_mult, void* stream);
int du_ds_loss_bwd(int mode, const float* const* logits, const int64_t* target, const int64_t* table, const float* coef,
                   const float* grad_out, float* const* dlogits, int B, int C, int H, int W, int S, const int* hs, const int* wd,
                   const float* weights, int has_ignore, int64_t ignore_label, void* stream);
/* DownsampleSegForDSTransform2 on the device: seg (B, H*W) int64 -> outs[s] (B, hs[s]*wd[s]) int64 for S in [1,4] maps (outs: HOST array
   of DEVICE pointers), by the index formula above, in one launch */
int du_downsample_seg(const int64_t* seg, int64_t* const* outs, int B, int H, int W, int S, const int* hs, const int* wd, void* stream);

/* ---- validation step (nnUNetTrainer.validation_step, nnUNetTrainer.py:946-1008 with get_tp_fp_fn_tn, dice.py:122-167): ONE read of the
        logits gives the sums of the matching training loss above (same layout and the same bits: run the matching *_finish on them) and the
        exact counts of the hard prediction.  counts (3, C) int64 = this step's [tp | fp | fn] over all C = K classes / R regions; accum
        (3, C) int64 += counts (NULL: none).  Prediction: argmax over K, lowest index among equal maxima (softmax modes); x > 0 (regions: the
        reference's sigmoid(x) > 0.5 except for 0 < x < ~1.2e-7, where torch's fp32 sigmoid rounds to 0.5).  Finite logits.  A pixel with the
        ignore label / ignore plane set adds to no count.  Integer arithmetic throughout, two stages, fixed order.  ws: *_ws_elems 4-byte
        elements.  DU_ERR_UNSUPPORTED for K outside [2,8], R outside [1,8] or B * HW >= 2^31 (int32 block partials). ---- */
int64_t du_val_dice_ce_ws_elems(int B, int K, int64_t HW);
int du_val_dice_ce(const float* logits, const int64_t* target, float* sums, int64_t* counts, int64_t* accum, int B, int K, int64_t HW,
                   float* ws, int64_t ws_elems, void* stream);
int64_t du_val_dice_ce_masked_ws_elems(int B, int K, int64_t HW);
int du_val_dice_ce_masked(const float* logits, const int64_t* target, float* sums, int64_t* counts, int64_t* accum, int B, int K,
                          int64_t HW, int64_t ignore_label, float* ws, int64_t ws_elems, void* stream);
int64_t du_val_dice_bce_ws_elems(int B, int R, int64_t HW);
int du_val_dice_bce(const float* logits, const uint8_t* target, float* sums, int64_t* counts, int64_t* accum, int B, int R, int64_t HW,
                    int has_ignore, float* ws, int64_t ws_elems, void* stream);

/* ---- FAPM FiLM modulation (dinounet_training.py:427-429): z = gamma * z_specific + beta; gb (rows,2R) = [gamma|beta], z2 (rows,2R) =
        [z_shared|z_specific], z (rows,R).  Backward writes all of dgb and the z_specific half of dz2. ---- */
int du_film_fwd(int dtype, const void* gb, const void* z2, void* z, int64_t rows, int R, void* stream);
int du_film_bwd(int dtype, const void* dz, const void* gb, const void* z2, void* dgb, void* dz2, int64_t rows, int R, void* stream);

/* ---- elementwise helpers --------------------------------------------------------------------------- */
/* SwiGLU gate of an interleaved projection u (rows, 2h): out (rows, h) = silu(u[:, 2j]) * u[:, 2j+1]   (layers/ffn_layers.py:73-77) */
int du_swiglu_pairs(int dtype, const void* u, void* out, int64_t rows, int64_t h, void* stream);
/* whole samples of an fp32 (B, n_per_sample) tensor by int64 index: scatter = 0: dst[j] = src[idx[j]], 1: dst[idx[j]] = src[j]
   (batch-subset stochastic depth of the ViT-7B blocks in train mode, layers/block.py:126-187) */
int du_sample_copy(const float* src, float* dst, const int64_t* idx, int k, int64_t n_per_sample, int scatter, void* stream);
int du_cast(int src_dtype, int dst_dtype, const void* src, void* dst, int64_t n, void* stream);
/* number of slabs a DU_STORE_SLABS product with contraction K asked to run `split_k` ranges actually writes (each range is rounded up
   to whole K tiles of the engine; empty ranges are dropped): what the caller passes to du_splitk_reduce_bf16 as `splits` */
int du_gemm_slab_count(int K, int split_k);
/* out[i] = bf16( sum_{s < splits, in order} slabs[s * n + i] ): the second half of a DU_STORE_SLABS split-K product (n % 4 == 0) */
int du_splitk_reduce_bf16(const float* slabs, void* out, int splits, int64_t n, void* stream);
/* NCHW fp32 image -> NHWC `dtype` with channels zero-padded to Cpad */
int du_nchw_to_nhwc_pad(int dst_dtype, const float* src, void* dst, int B, int C, int H, int W, int Cpad, void* stream);
/* NHWC `dtype` (pixel stride ld) -> NCHW fp32 */
int du_nhwc_to_nchw_f32(int src_dtype, const void* src, int64_t ld, float* dst, int B, int C, int H, int W, void* stream);
/* 16x16/s16 patch gather: NCHW fp32 image -> (B*h*w, C*256) rows ordered (c, dy, dx) like Conv2d weight.flatten(1) */
int du_patchify16(int dst_dtype, const float* src, void* dst, int B, int C, int H, int W, void* stream);

/* One launch that turns every trainable fp32 weight into its kernel-ready form (bf16 cast / im2col column order / flipped data-gradient
   order / ConvTranspose layouts / concatenations).  table: n rows of 8 int64 on the DEVICE [src, dst, kind | dst_is_f32 << 8, A, B, T,
   Cp, n_out] (kinds: see elementwise.hip), bprefix: n+1 exclusive prefix sums of ceil(n_out / 4096) = workgroups per row. */
int du_pack_weights(const int64_t* table, const int64_t* bprefix, int n, int64_t nblocks, void* stream);

/* ---- GPU-side training augmentation for 2D slices: the transforms of nnUNetTrainer.get_training_transforms
   (dinounet/training/nnUNetTrainer/nnUNetTrainer.py:684-776; the reference delegates them to the un-vendored `batchgenerators` package:
   parity unpinned, algorithms restated from the package, see csrc/augment.hip).  All tensors NCHW fp32 on the device; a "plane" is one
   (sample, channel) image of n = H * W elements; per-plane parameter arrays live on the device. -------------------------------------- */
/* SpatialTransform (rotation + isotropic scale + centre crop) and MirrorTransform in one resampling pass.  params (B, 6) =
   [m00, m01, m10, m11, flip_y, flip_x]: input coordinate = input centre + M (output coordinate - output centre), M = scale * R(angle).
   data (B,C,Hi,Wi) -> data_out (B,C,Ho,Wo) bicubic, zero outside; seg (B,1,Hi,Wi) (nullable) -> seg_out by the order-1 label rule. */
int du_aug_spatial(const float* data, const float* seg, const float* params, float* data_out, float* seg_out, int B, int C, int Hi, int Wi,
                   int Ho, int Wo, void* stream);
/* stats (planes, 4) = mean, population std, min, max of every plane (n % 4 == 0); two passes, mean and std err relative to the
   plane's spread whatever its offset */
int du_aug_plane_stats(const float* x, float* stats, int planes, int64_t n, void* stream);
/* GaussianNoiseTransform + BrightnessMultiplicativeTransform: x = (x + sigma[p] * N(0,1)) * mult[p]   (sigma 0 / mult 1 = off) */
int du_aug_noise_mult(float* x, const float* sigma, const float* mult, int planes, int64_t n, int seed, void* stream);
/* ContrastAugmentationTransform (preserve_range): x = clip((x - mean) * factor[p] + mean, min, max), stats of the current contents */
int du_aug_contrast(float* x, const float* factor, const float* stats, int planes, int64_t n, void* stream);
/* GammaTransform body on x (or on -x where invert[p] != 0): ((v - min) / (range + 1e-7))^gamma[p] * range + min; gamma <= 0 = off.
   retain_stats and the final negation are a du_aug_plane_stats + du_aug_affine pair */
int du_aug_gamma(float* x, const float* gamma, const float* invert, const float* stats, int planes, int64_t n, void* stream);
int du_aug_affine(float* x, const float* a, const float* b, int planes, int64_t n, void* stream);
/* GaussianBlurTransform: one separable pass along axis 0 (y) / 1 (x), radius int(4 sigma + 0.5), reflect borders; sigma[p] <= 0 copies */
int du_aug_blur(const float* x, float* y, const float* sigma, int planes, int H, int W, int axis, void* stream);
/* SimulateLowResolutionTransform: nearest-neighbour down to round(size * zoom[p]), cubic back up; zoom outside (0, 1) copies */
int du_aug_lowres(const float* x, float* y, const float* zoom, int planes, int H, int W, void* stream);
/* ---- The same transforms with the interpolation batchgenerators calls (GPUAugment2D(interpolation="spline"), csrc/augment_spline.hip):
   fp64 arithmetic, one rounding at the store.  Every entry: DU_ERR_BAD_ARG for a NULL pointer or a size < 1, DU_ERR_UNSUPPORTED for a
   plane of 2^31 elements or more, nothing launched in either case. ---- */
/* Cubic B-spline coefficients (scipy spline_filter, order 3, mode "mirror") of planes plane_idx[0 .. planes) of x (in_planes, H, W):
   ws[j] (H, W) fp64 for j < planes; ws holds du_aug_spline_ws_elems(planes, H, W) = 2 planes H W doubles (the second half is the row
   pass's result).  du_aug_spline_ws_elems launches nothing and returns the (negative) code itself for a bad shape. */
int64_t du_aug_spline_ws_elems(int planes, int H, int W);
int du_aug_spline_coeffs(const float* x, int in_planes, const int32_t* plane_idx, int planes, int H, int W, double* ws, int64_t ws_elems,
                         void* stream);
/* du_aug_spatial with map_coordinates(order=3, mode="constant", cval=0) for the image: a pixel whose coordinate leaves [0, Hi - 1] x
   [0, Wi - 1] is 0, inside it is the 4 x 4 B-spline sum over coef (coef_planes, Hi, Wi), slots[b * C + c] naming the plane's coefficients,
   tap indices mirrored.  Labels: the largest label, -1 included, whose bilinear weight reaches 1/2, else 0: seg_out may hold -1
   (du_aug_mask).  A sample whose matrix is exactly [1, 0, 0, 1] is the integer centre crop, lower bounds (Hi - Ho) // 2, (Wi - Wo) // 2,
   of image and labels, flipped; its slots are not read. */
int du_aug_spatial_spline(const float* data, const float* seg, const float* params, const double* coef, int coef_planes,
                          const int32_t* slots, float* data_out, float* seg_out, int B, int C, int Hi, int Wi, int Ho, int Wo, void* stream);
/* du_aug_lowres with skimage's resize going up (scipy zoom(order=3, mode="nearest", grid_mode=True), clipped to the low grid's range).
   sizes (planes, 2) int32 on the device = the low grid (Hl, Wl) <= (H, W) of every plane, (0, 0) = copy the plane.  Scratch: bounds
   (planes, 32, 2) fp32 (partial min / max of the low grids), tmp planes H W doubles.  planes <= 65535. */
int du_aug_lowres_spline(const float* x, float* y, const int32_t* sizes, float* bounds, double* tmp, int planes, int H, int W, void* stream);
/* MaskTransform + RemoveLabelTransform(-1, 0): where labels (B, 1, n) < 0, the channels c of data (B, C, n) with bit c of channel_bits
   set become 0 and the label becomes 0.  DU_ERR_BAD_ARG for a bit at or above C (channels 0 .. 62 can be masked). */
int du_aug_mask(float* data, float* labels, int64_t channel_bits, int B, int C, int64_t n, void* stream);

/* Segmentation head (the decoder's last 1x1 convolution, 32 channels -> K <= 4 classes; dinounet_training.py:603-629, nnU-Net UNetDecoder
   seg_layers): one streaming pass instead of a padded GEMM + layout passes.  bf16 activations, weights rounded to bf16 as autocast does.
   du_seg_head_fwd: x (B, HW, 32) NHWC bf16 (pixel stride ldx), w (K, 32) fp32, bias (K) fp32 or null -> out (B, K, HW) fp32 (NCHW logits).
   du_seg_head_bwd: dl (B, K, HW) fp32 -> dx (B, HW, 32) bf16 (nullable), dwb = [dw (K, 32), db (K)] fp32 (K * 33 floats rounded up to an
   even count, OVERWRITTEN); part = du_seg_head_bwd_blocks(B, HW) rows of that length, scratch.  DU_ERR_UNSUPPORTED for other C / K. */
int du_seg_head_fwd(const void* x, int64_t ldx, const float* w, const float* bias, float* out, int B, int64_t HW, int C, int K, void* stream);
int du_seg_head_bwd_blocks(int B, int64_t HW);
int du_seg_head_bwd(const void* x, int64_t ldx, const float* w, const float* dl, void* dx, int64_t lddx, float* part, float* dwb, int B,
                    int64_t HW, int C, int K, void* stream);

/* library self-description */
const char* du_version(void);
int du_device_ok(void); /* 1 if the current device is gfx950 */
/* Kernel-selection knobs for measurement tools (within-process A/B runs, tools/gemm_p8_bench.py); results never depend on them.
   key 0: 256 x 256 multi-phase NT GEMM (gemm_p8.hip): -1 heuristic (default), 0 never, 1 wherever legal;
   key 1: its pinned issue order on (1, default) / off (0);  key 2: its tile band height (default 4);
   key 3: epilogue ablations of those kernels (timing only);  key 4: attention tile-program ablation bits (0 = the product kernel; tools/attn_ablate.py);
   key 5: weight gradients (contraction-major operands, split-K) on the multi-phase kernel: 1 where it pays (default), 2 wherever legal,
          0 never (the 128 x 128 kernel);
   key 10: the persistent 256 x 128 NT kernel: 1 where its cost model wins (default), 0 never, 2 wherever legal;
   key 12: the resident-weights streaming kernel for K <= 256 (csrc/gemm_rk.hip): 1 = K <= 192 (default), 2 = K = 256 too, 0 = never;
   key 13: 3 x 3 weight gradients (du_conv3x3_wgrad_halo): 1 = the round-5 kernel for 32 / 64 output channels (default), 2 = for 128 too,
           0 = the round-3 one;
   key 15: the <= 64 ragged rows behind the last full 256-row tile of a tall NT product (the ViT: M = 8 x 1029): 0 = by extra workgroups
           behind the tile grid (default), 1 = by the tile workgroups themselves once their tiles are done;
   key 16: fp32-result NT products with 64-128 tiles of 256 x 256 and K >= 1024 (the ViT's proj / fc2) as K-split pairs of workgroups that
           exchange fp32 halves inside the launch (needs du_gemm_args.ks_ws): 0 = off (default), 1 = on;
   key 17: the ragged-row units of a product with K >= 2048 on the one-shot tile kernels (the ViT's fc2) as (32 columns, K slice) pairs that
           meet through du_gemm_args.ks_ws: 1 (default), 0 = one unit per 32 columns walks the whole contraction;
   key 18: du_layernorm_fwd with two rows per wave: 1 = where the rows overflow one round of waves (32 per CU) by less than 2x -- the ViT's
           8232 rows (default), 0 = never, 2 = always;
   key 19: depthwise 3 x 3 on the band kernels (dwconv.hip) where the plan of du_dwconv3x3_* allows: 1 (default), 0 = the kernels of
           elementwise.hip everywhere (du_dwconv3x3_plan_describe then names a row kernel); tuning aid: bits 0-7 >= 2 = bands of that many rows in forward and data
           gradient, bits 8-15 >= 2 = in the weight gradient, instead of the height the library picks;
   key 14: bf16 products with a bf16 residual on the persistent kernel (the residual as two more K-steps): 1 (default), 0 = one-shot kernels;
   key 9: number of independent products the caller keeps in flight on DIFFERENT streams (default 1; dinounet_amd runs the frozen ViT as
          two half-batch chains): du_gemm's tile choice then counts workgroup rounds on 256 / value CUs. */
int du_set_option(int key, int value);
/* tuning aid: the 8 per-segment cycle sums of the last probed attention launch (du_set_option(4, bits | 64), tools/attn_ablate.py) */
int du_debug_attn_probe(uint64_t* host8);
/* tuning aid: workgroups per CU the runtime's occupancy query admits for an attention kernel (0: 64 queries per wave, d_head 64;
   1: d_head 128; 2: the round-3 kernel) */
int du_debug_attn_occupancy(int which);
/* tuning aid: 8 words (loop begin tick, loop end tick, HW_ID, XCC_ID, kernel entry tick, exit tick, 2 spare) of the first n (<= 1024) workgroups
   of the last probed launch of the 64-queries-per-wave kernel */
int du_debug_attn_census(uint64_t* host, int n);

/* ---- sliding-window inference: predicted_logits[sl] += prediction * gaussian; n_predictions[sl] += gaussian
   (dinounet/inference/predict_from_raw_data.py:607-608) for a batch of nb windows, then predicted_logits /= n_predictions (:610).
   pred (K, D, H, W) and npred (D, H, W) fp32 accumulators, zero-initialised by the caller before the first window; n = D * H * W. */
int du_window_normalize(float* pred, const float* npred, int K, int64_t n, void* stream);
/* The accumulation runs over a LIST of cases (a single case is a list of one), one window batch holding windows of several of them
   (csrc/window.hip).  All tables are DEVICE arrays:
   geom (ncases, 3) int32 = (D, H, W) of each case; desc (nb, 4) int32 on 16 bytes = (case, d, y0, x0) of each window, y0 / x0 in the case's
   padded frame Hp = max(H, ph), lo_y = (Hp - H) / 2, likewise x (pad_nd_image: centred, the odd pixel on the high side).
   du_window_gather: cases = table of ncases pointers to contiguous fp32 (C, D, H, W) volumes; x (slots, C, ph, pw) fp32 = the windows, a source
   position outside the image reads as 0, slots nb .. slots-1 are written as zeros.  A pure copy.
   du_window_accumulate_cases: logits (nb, K, ph, pw), gauss (ph, pw); preds / npreds = tables of the cases' accumulators (K, D, Hp, Wp) and
   (D, Hp, Wp).  No float atomics: every accumulator element is read once, gets acc = fadd(acc, fmul(logit, g)) (npred: acc + g) of every
   covering slot of the launch in slot order, and is written once -- equal to the reference's sequential loop in fp32 to the bit when a case's
   windows arrive in its order (launches of one stream are ordered).  A descriptor that does not fit its case is skipped (gather: zeros).
   DU_ERR_BAD_ARG: a NULL pointer, a non-positive size, slots < nb, desc not on 16 bytes; DU_ERR_UNSUPPORTED: nb > 64 (accumulate), ph pw >=
   2^29; both before any launch. */
int du_window_gather(const void* const* cases, const int32_t* geom, const int32_t* desc, float* x, int ncases, int nb, int slots, int C,
                     int ph, int pw, void* stream);
int du_window_accumulate_cases(const float* logits, const float* gauss, const int32_t* desc, const int32_t* geom, float* const* preds,
                               float* const* npreds, int ncases, int nb, int K, int ph, int pw, void* stream);

/* ---- export tail: accumulators -> label map in the case's original geometry, in ONE pass
   (convert_predicted_logits_to_segmentation_with_correct_shape, dinounet/inference/export_prediction.py:15-68, with
   LabelManager.convert_probabilities_to_segmentation / revert_cropping_on_probabilities, utilities/label_handling/label_handling.py:143-175,
   185-209).  sums (K, D, Hp, Wp) fp32 = the un-normalised predicted_logits of du_window_accumulate_cases, npred (D, Hp, Wp) fp32 (NULL = 1:
   finished logits); (y0, x0, Hc, Wc) the un-padding window inside (Hp, Wp); (Ho, Wo) = shape_after_cropping_and_before_resampling[1:];
   (D0, H0, W0) = shape_before_cropping, (bd, by, bx) the low corner of bbox_used_for_cropping, whose size is (D, Ho, Wo).
   seg (D0, H0, W0) uint8, written in full (0 outside the bbox); probs (K, D0, H0, W0) fp32 or NULL (outside the bbox: plane 0 = 1 in softmax
   mode, all 0 in region mode).  mode DU_EXPORT_SOFTMAX (K in [2,8]): argmax, lowest index among equal maxima; DU_EXPORT_REGIONS (K = R in
   [1,8]): byte i of region_order is regions_class_order[i], the label is that of the LARGEST i with logit_i > 0, else 0 (the overwrite
   loop of label_handling.py:170-171; x > 0 for sigmoid(x) > 0.5 as in the validation step above).  (Ho, Wo) == (Hc, Wc): the raw sums are
   compared, no arithmetic.  Otherwise order-1 interpolation of sums / npred at 4 taps, edge clamp, source position from integers:
   n = (2 dst + 1) Hc - Ho, tap floor(n / 2 Ho), weight (n mod 2 Ho) / (2 Ho).  Slices are independent.  flag (DEVICE int32, zeroed by the
   caller) = 1 if a sums / npred element read for a voxel inside the window is not finite (predict_from_raw_data.py:612-615).
   DU_ERR_UNSUPPORTED: K out of range; DU_ERR_BAD_ARG: window outside (Hp, Wp), bbox outside (D0, H0, W0). */
#define DU_EXPORT_SOFTMAX 0
#define DU_EXPORT_REGIONS 1
int du_export_seg(const float* sums, const float* npred, uint8_t* seg, float* probs, int32_t* flag, int K, int D, int Hp, int Wp, int y0,
                  int x0, int Hc, int Wc, int Ho, int Wo, int D0, int H0, int W0, int bd, int by, int bx, int mode, int64_t region_order,
                  void* stream);
/* per-case counts (compute_tp_fp_fn_tn with region_or_label_to_mask, dinounet/evaluation/evaluate_predictions.py:75-94, 176-186): pred,
   ref (n) uint8 label maps, masks (R) int64 DEVICE bit masks as in du_labels_to_regions (labels 0..63, any other label is in no region),
   counts (4, R) int64 = tp | fp | fn | tn over the voxels with ref != ignore_label (has_ignore).  Integers, two stages, fixed order.
   ws: du_seg_counts_ws_elems int32 elements.  DU_ERR_UNSUPPORTED for R outside [1,8] or n >= 2^31. */
int64_t du_seg_counts_ws_elems(int64_t n, int R);
int du_seg_counts(const uint8_t* pred, const uint8_t* ref, const int64_t* masks, int64_t* counts, int64_t n, int R, int has_ignore,
                  int ignore_label, int32_t* ws, int64_t ws_elems, void* stream);

/* ---- ensembling: M member probability volumes -> label map (+ the averaged probabilities), ONE pass (csrc/ensemble.hip;
   average_probabilities and merge_files, dinounet/ensembling/ensemble.py:17-46).  members: DEVICE table of M (1..16) pointers, each to a
   contiguous (K, n) array, all fp32 (elem_size 4) or all fp16 (elem_size 2); a member may start at any element.
   mean (K, n) fp32 or NULL = (((p0 + p1) + p2) + ...) / M in fp32, members in table order, one correctly rounded division: equal to numpy's
   `avg += p; avg /= M` to the bit for finite inputs.  seg (n) uint8 or NULL (then K may be 1 in either mode): DU_EXPORT_SOFTMAX (K in [2,8])
   the lowest index among the maxima of the mean; DU_EXPORT_REGIONS (K = R in [1,8]) byte i of region_order painted where mean_i > 0.5, in
   order (convert_probabilities_to_segmentation, label_handling.py:143-175).  flag (DEVICE int32, zeroed by the caller) = 1 if a mean is
   not finite (a non-finite member always makes one).  16-byte loads when every member pointer is on 16 bytes, n is a multiple of
   16 / elem_size and seg / mean are aligned likewise; guarded element accesses otherwise.  DU_ERR_UNSUPPORTED: M, K, elem_size out of
   range or n < 0; DU_ERR_BAD_ARG: a NULL table or flag, neither seg nor mean, an unknown mode. */
int du_ensemble_merge(const void* const* members, int M, int elem_size, int K, int64_t n, int mode, int64_t region_order, uint8_t* seg,
                      float* mean, int32_t* flag, void* stream);

/* ---- fused clip_grad_norm_ + Nesterov SGD over all trainable tensors (replaces
   torch.nn.utils.clip_grad_norm_(params, 12) + torch.optim.SGD.step(), dinounet/training/nnUNetTrainer/nnUNetTrainer.py:486,922-924).
   table: n_tensors rows of 4 x int64 [param ptr, grad ptr, momentum-buffer ptr, numel] (fp32 tensors, contiguous);
   bprefix[i] = first workgroup of row i, bprefix[n_tensors] = nblocks, 4096 elements per workgroup;
   hyper (DEVICE, fp32): [lr, momentum, weight_decay, max_norm, nesterov (0/1)] -- read at run time, so a captured graph follows a
   learning-rate schedule; ws: du_clip_sgd_ws_elems(nblocks) floats, ws[nblocks] = total gradient norm, ws[nblocks+1] = clip coefficient
   on return.  Gradients are scaled in place by the coefficient (as clip_grad_norm_ does); zero-filled momentum buffers on the first
   step reproduce torch's "buf = d_p". */
int64_t du_clip_sgd_ws_elems(int nblocks);
int du_clip_sgd(const int64_t* table, const int64_t* bprefix, int n_tensors, int nblocks, const float* hyper, float* ws,
                int64_t ws_elems, void* stream);

/* ---- surface metrics: border voxels and the exact Euclidean distance transform of their complement (csrc/surface.hip; HD95 / ASD of
   compute_surface_distances, evaluate_predictions.py:97-149, i.e. medpy.metric.hd95 / asd).  Volumes are (D, H, W), every extent in
   [1, 1024] (DU_ERR_UNSUPPORTED beyond: offsets and indices are 10-bit fields); spacings (sz, sy, sx) positive, in array-axis order.
   du_surface_border: pred / ref uint8 label maps, masks (R <= 8) int64 DEVICE bit masks as in du_seg_counts.  bits (D, H, W) uint16: bit r =
   the voxel is a border voxel of region r of pred, bit 8 + r = of ref (a mask voxel with one of its six face neighbours outside the mask or
   outside the volume).  counts (4, R) int64 DEVICE = mask voxels pred | mask voxels ref | border voxels pred | border voxels ref, exact.
   ws: du_surface_border_ws_elems int32 elements.
   du_surface_field: field (D, H, W) fp64 = the squared distance (dz sz)^2 + (dy sy)^2 + (dx sx)^2 (added in that order) to the nearest
   voxel with bit `bit` of `bits`, +inf if there is none.
   du_surface_gather: for every region r with bit r of `active`: the ref field at the pred border voxels -> dist_sq[seg_off[2r] ..
   seg_off[2r + 1]) and sqrt_sums[r] = the sum of their square roots (fixed order, no float atomics); the pred field at the ref border voxels
   -> dist_sq[seg_off[2r + 1] .. seg_off[2r + 2]).  seg_off: 2R + 1 int64 on the HOST (read during the call), from the border counts; the
   order inside a segment is not defined.  dist_sq, sqrt_sums (R) fp64 DEVICE.
   ws of both: du_surface_ws_elems(D, H, W) 8-byte elements, 8-byte aligned = ceil(n / 4) + ceil(n / 2) + H * ceil(W / c) + 8, n = D H W,
   c = the largest power of two <= 64 with c * D * 4 <= 65536 (6 bytes per voxel: one uint16 and one uint32 field, whatever R is). ---- */
int64_t du_surface_border_ws_elems(int64_t n, int R);
int du_surface_border(const uint8_t* pred, const uint8_t* ref, const int64_t* masks, uint16_t* bits, int64_t* counts, int D, int H, int W,
                      int R, int32_t* ws, int64_t ws_elems, void* stream);
int64_t du_surface_ws_elems(int D, int H, int W);
int du_surface_field(const uint16_t* bits, double* field, int D, int H, int W, int bit, double sz, double sy, double sx, void* ws,
                     int64_t ws_elems, void* stream);
int du_surface_gather(const uint16_t* bits, int D, int H, int W, int R, int active, double sz, double sy, double sx,
                      const int64_t* seg_off_host, double* dist_sq, double* sqrt_sums, void* ws, int64_t ws_elems, void* stream);

/* ---- connected components of one mask of a label map, and "keep only the largest" (csrc/cc.hip;
   remove_all_but_largest_component_from_segmentation, dinounet/postprocessing/remove_connected_components.py:22-34).  seg (D, H, W) uint8,
   read-only; a voxel is in the mask if its label is < 64 and bit `label` of mask_bits is set (the du_labels_to_regions convention: the OR of
   the masks of a list of labels / regions; any other label is in no mask).  Full connectivity: 26 neighbours (8 in-plane with D == 1, fewer
   along any axis of extent 1).  The id of a component is the smallest linear index (z H + y) W + x of its voxels, so the labelling depends
   on the input alone; the largest component has the most voxels, on a tie the smallest id (the first in raster order).
   du_cc_label: ids (D, H, W) int32 = the id of the voxel's component, -1 outside the mask; stats (3) int64 DEVICE = {n_components, size of
   the largest, id of the largest or -1 without one}.
   du_cc_keep_largest: out (D, H, W) uint8, every voxel written = background_label (0..255) where the voxel is in the mask but not in the
   largest component, else seg; an empty mask copies seg.  out must not overlap seg (DU_ERR_BAD_ARG).  stats as above.
   ws: du_cc_ws_elems(D, H, W, keep) int32 elements, 16-byte aligned, keep = 0 for du_cc_label, 1 for du_cc_keep_largest
   = 4 + (2 + keep) * n4, n4 = D H W rounded up to a multiple of 4: parent and size fields (8 bytes per voxel), for keep_largest the
   ids too (12 bytes per voxel).  Five kernels and one 16-byte memset on `stream` (six kernels for keep_largest), none waits for another workgroup; integer atomics
   only, so results are bit-identical from run to run.
   DU_ERR_UNSUPPORTED: D H W >= 2^31.  DU_ERR_BAD_ARG: a NULL pointer, an extent < 1, ws misaligned or ws_elems below du_cc_ws_elems (which
   is 0 for a shape with an error). ---- */
int64_t du_cc_ws_elems(int D, int H, int W, int keep);
int du_cc_label(const uint8_t* seg, int64_t mask_bits, int32_t* ids, int64_t* stats, int D, int H, int W, int32_t* ws, int64_t ws_elems,
                void* stream);
int du_cc_keep_largest(const uint8_t* seg, int64_t mask_bits, int background_label, uint8_t* out, int64_t* stats, int D, int H, int W,
                       int32_t* ws, int64_t ws_elems, void* stream);

/* ---- preprocessing of a raw case (csrc/preprocess.hip; DefaultPreprocessor.run_case_npy,
   dinounet/preprocessing/preprocessors/default_preprocessor.py:40-118): crop to the non-zero region, normalise, resample in-plane.  Every
   launch goes on `stream`; no call reads anything back.
   du_pre_nonzero_mask: data (C, D, H, W) of dtype DU_PRE_*, read-only -> mask (D, H, W) uint8 = binary_fill_holes(OR_c data[c] != 0) with
   scipy's default structure: a zero voxel is filled exactly when its 6-connected component of zero voxels touches no face of the volume
   (so nothing is filled with D <= 2).  bbox (6) int32 DEVICE = {z lo, y lo, x lo, z hi, y hi, x hi}, half open, of the filled mask; hi = 0
   for an all-zero case.  ws: du_pre_fill_ws_elems(D, H, W) int32 elements, 16-byte aligned = D H W + 1 rounded up to 4: the union-find
   parents of the zero voxels, shifted by one, word 0 = the node "outside the volume".  Three kernels and two memsets; integer atomics only.
   DU_ERR_UNSUPPORTED: D H W >= 2^31 - 1 or an unknown dtype.
   du_pre_crop: one pass over the box [z0, z0 + d) x [y0, y0 + h) x [x0, x0 + w): out (C, d, h, w) fp32 = data converted; seg_out (d, h, w)
   int16 = with seg (D, H, W) int16: seg, but nonzero_label where seg == 0 outside the mask; without (NULL): nonzero_label outside the
   mask, 0 inside.
   du_pre_plane_stats: img (C, D, HW) fp32, seg (D, HW) int16 or NULL -> plane_minmax (C D, 2) fp32 = min and max of every channel slice;
   chan_stats (C, 5) fp64 = {min, max, sum, count, -} of every channel volume, sum and count over the voxels with seg >= 0 (all voxels
   without seg), the sum in fp64 in a fixed order.  du_pre_sq_dev: chan_stats[c][4] = the fp64 sum over the same voxels of
   (x - sum / count)^2, a second pass.  ws of both: du_pre_stats_ws_elems(C, D, HW) fp64 elements.
   du_pre_normalize: ONE channel volume img (n) fp32 in place, seg (n) int16 or NULL, chan_stats = the 5 doubles of this channel:
     DU_PRE_NORM_NONE     nothing
     DU_PRE_NORM_RGB      x / 255 (fp32 divide)
     DU_PRE_NORM_CT       (min(max(x, p0), p1) - p2) / p3 in fp32, every step rounded (NaN stays NaN)
     DU_PRE_NORM_RESCALE  (x - min) / max(fp32(max - min), 1e-8f) in fp32
     DU_PRE_NORM_ZSCORE   fp32((double(x) - mean) / max(std, 1e-8)), mean = sum / count, std = sqrt(sq_dev / count); with seg only where
                          seg >= 0, every other voxel keeps its bits
   du_pre_resize_cubic: in (P, H, W) fp32 -> out (P, Ho, Wo) fp32 = skimage.transform.resize(order 3, mode 'edge', anti_aliasing False)
   of every plane: scipy.ndimage.zoom(order 3, mode 'nearest', grid_mode True), then a clip to bounds (P, 2) fp32 = {lo, hi} of the plane.
   fp64 throughout, one rounding to fp32.  An axis whose extent does not change is not touched.  tmp: P H Wo fp64 when both axes change,
   else unused (may be NULL).  DU_ERR_BAD_ARG if neither axis changes.
   du_pre_resize_seg: in (D, H, W) int16 -> out (D, Ho, Wo) int16 = resize_segmentation(order 1) in integers: the largest label whose
   bilinear one-hot weight is >= 1/2, else 0. ---- */
#define DU_PRE_F32 0
#define DU_PRE_F64 1
#define DU_PRE_U8 2
#define DU_PRE_I16 3
#define DU_PRE_I32 4
#define DU_PRE_NORM_NONE 0
#define DU_PRE_NORM_RGB 1
#define DU_PRE_NORM_CT 2
#define DU_PRE_NORM_RESCALE 3
#define DU_PRE_NORM_ZSCORE 4
int64_t du_pre_fill_ws_elems(int D, int H, int W);
int du_pre_nonzero_mask(const void* data, int dtype, int C, int D, int H, int W, uint8_t* mask, int32_t* bbox, int32_t* ws,
                        int64_t ws_elems, void* stream);
int du_pre_crop(const void* data, int dtype, const uint8_t* mask, const int16_t* seg, int C, int D, int H, int W, int z0, int y0, int x0,
                int d, int h, int w, int nonzero_label, float* out, int16_t* seg_out, void* stream);
int64_t du_pre_stats_ws_elems(int C, int D, int64_t HW);
int du_pre_plane_stats(const float* img, const int16_t* seg, float* plane_minmax, double* chan_stats, int C, int D, int64_t HW, double* ws,
                       int64_t ws_elems, void* stream);
int du_pre_sq_dev(const float* img, const int16_t* seg, double* chan_stats, int C, int D, int64_t HW, double* ws, int64_t ws_elems,
                  void* stream);
int du_pre_normalize(float* img, const int16_t* seg, const double* chan_stats, int scheme, float p0, float p1, float p2, float p3,
                     int64_t n, void* stream);
int du_pre_resize_cubic(const float* in, float* out, const float* bounds, double* tmp, int P, int H, int W, int Ho, int Wo, void* stream);
int du_pre_resize_seg(const int16_t* in, int16_t* out, int D, int H, int W, int Ho, int Wo, void* stream);

/* ---- training batches (csrc/dataload.hip): the class-location tables of DefaultPreprocessor._sample_foreground_locations
   (dinounet/preprocessing/preprocessors/default_preprocessor.py:157-181) and the batch gather of nnUNetDataLoader2D.generate_train_batch
   (dinounet/training/dataloading/data_loader_2d.py:46-85).  Every launch goes on `stream`; no call reads anything back.
   seg (D, H, W) int16, read-only, D H W < 2^31.  masks (G) int64 DEVICE: a voxel is a member of mask g if 0 <= label <= 63 and bit `label`
   of masks[g] is set (the du_labels_to_regions convention; any other label is in no mask).  Members are ranked in the raster order
   (z H + y) W + x, the order np.argwhere lists them in.
   du_dl_class_counts: ws (G, nchunks) int32 = per mask the exclusive prefix of the member counts of the chunks of 1024 consecutive voxels,
   nchunks = ceil(D H W / 1024); totals (G) int64 DEVICE = the member count of every mask.  Two kernels, no atomics.
   du_dl_select: ws as du_dl_class_counts left it for the same seg, masks and G; ranks (m) int64 DEVICE in any order, each in
   [0, totals[g]); out (m, 4) int32 = {0, z, y, x} of the member of mask g with that rank, i.e. np.argwhere(mask)[ranks] of the mask seen as
   (1, D, H, W).  A rank outside [0, totals[g]) gives {0, -1, -1, -1}.  One wave per rank: a binary search over the prefix, then ballots and
   popcounts over one chunk.
   ws: du_dl_ws_elems(D, H, W, G) int32 elements = G nchunks rounded up to 4, 16-byte aligned.
   DU_ERR_UNSUPPORTED: D H W >= 2^31.  DU_ERR_BAD_ARG: a NULL or misaligned pointer, an extent, G or m < 1, g outside [0, G), m > D H W, ws
   misaligned or ws_elems below du_dl_ws_elems.  du_dl_ws_elems launches nothing and returns that (negative) code itself for such a shape.
   du_dl_gather: one launch for a batch.  jobs (B, 8) int64 DEVICE, row b = {address of data (C, D, H, W) fp32, address of seg (D, H, W) int16,
   D, H, W, slice, y0, x0}; the cases may differ in D, H, W, not in C; y0 / x0 may be negative or run past the image.
   data_out (B, C, ph, pw) fp32 = data[:, slice, y0 : y0 + ph, x0 : x0 + pw], 0 outside the image; seg_out (B, 1, ph, pw) = the same window of
   seg, -1 outside: int16, or fp32 with seg_f32 != 0 (what du_aug_spatial takes).  A row whose slice is outside [0, D) reads as outside
   everywhere.  The inputs are not modified.  DU_ERR_BAD_ARG: NULL or misaligned pointer, B, C, ph or pw < 1. ---- */
int64_t du_dl_ws_elems(int D, int H, int W, int G);
int du_dl_class_counts(const int16_t* seg, const int64_t* masks, int G, int D, int H, int W, int32_t* ws, int64_t ws_elems, int64_t* totals,
                       void* stream);
int du_dl_select(const int16_t* seg, const int64_t* masks, int G, int g, int D, int H, int W, const int32_t* ws, int64_t ws_elems,
                 const int64_t* ranks, int64_t m, int32_t* out, void* stream);
int du_dl_gather(const int64_t* jobs, int B, int C, int ph, int pw, float* data_out, void* seg_out, int seg_f32, void* stream);

/* ---- dataset fingerprint (csrc/fingerprint.hip): the foreground statistics and samples of DatasetFingerprintExtractor
   (dinounet/experiment_planning/dataset_fingerprint/fingerprint_extractor.py:42-80 per case, :156-177 over the dataset).  Every launch goes
   on `stream`; no call reads anything back.
   img (C, n) fp32 and seg (n) int16 or NULL, read-only, n < 2^31, C <= 65535.  An element is a member if seg > 0; with NULL every element
   is (the dataset-level form over the concatenated samples).  Every channel has the same members.
   du_fp_moments: stats (C, 6) fp64 DEVICE = {member count, min, max, sum, count of NaN members, -}.  mode 0 writes the first five and
   zeroes the sixth: the sum in fp64 in a fixed order (per lane in sequence, lanes by the xor tree, waves and stretches in order), min and
   max over the members that are not NaN, +inf and -inf without members.  mode 1 reads count and sum and writes stats[c][5] = the fp64 sum
   of (x - sum / count)^2 over the members, the second pass.  Two kernels each, no atomics.
   du_fp_order_stats: ranks (C, R) int64 DEVICE, 1 <= R <= 8, each in [0, count); out (C, R) fp32 = the member of channel c whose 0-based
   position in ascending order is ranks[c][r], i.e. np.sort(members)[rank], -0.0 sorted below +0.0.  Radix select over the order-preserving
   32-bit key, 8 bits a pass: four sweeps over img and seg, each followed by a one-workgroup kernel per channel; all C R targets are
   served by the same sweeps.  Integer atomics only.  The ranks live on the device, so the call cannot refuse one: a rank outside
   [0, count) gives NaN in its place and disturbs no other target.
   du_fp_sample: ranks (C, m) int64 DEVICE in the raster order of the members, in any order, repeats allowed; out (C, m) fp32 =
   img[c][members[ranks[c][j]]], i.e. images[c][mask][ranks[c]].  With seg: member counts of the chunks of 1024 elements, their exclusive
   prefix, then one wave per rank (du_dl_select's scheme with the predicate seg > 0); without: a plain gather.  A rank outside [0, count)
   gives NaN.
   ws of all three: du_fp_ws_elems(C, n) int32 elements, 16-byte aligned; the calls of one stream may share it, nothing is kept in it
   between calls.  DU_ERR_UNSUPPORTED: n >= 2^31, C > 65535, or m >= 2^40 (du_fp_sample).  DU_ERR_BAD_ARG: a NULL (seg excepted) or misaligned pointer, C, n or m < 1,
   R outside 1..8, mode outside {0, 1}, ws_elems below du_fp_ws_elems.  du_fp_ws_elems launches nothing and returns that (negative) code
   itself for such a shape. ---- */
int64_t du_fp_ws_elems(int C, int64_t n);
int du_fp_moments(const float* img, const int16_t* seg, int C, int64_t n, int mode, double* stats, int32_t* ws, int64_t ws_elems,
                  void* stream);
int du_fp_order_stats(const float* img, const int16_t* seg, int C, int64_t n, const int64_t* ranks, int R, float* out, int32_t* ws,
                      int64_t ws_elems, void* stream);
int du_fp_sample(const float* img, const int16_t* seg, int C, int64_t n, const int64_t* ranks, int64_t m, float* out, int32_t* ws,
                 int64_t ws_elems, void* stream);

#ifdef __cplusplus
}
#endif
#endif
