/*
 * scflow_hip.h — C ABI of the MI355X (gfx950) SCFlow refinement hot path.
 *
 * One shared library, libscflow_hip.so (scflow_amd/lib/), built with
 * `hipcc --offload-arch=gfx950`.  Every entry point:
 *   - takes plain device pointers (fp32 unless stated), sizes and a hipStream_t passed as void*;
 *   - enqueues work on that stream and returns immediately (no host sync, no allocation, so
 *     callers may capture the calls into a hipGraph);
 *   - returns 0 on success, a negative SCFLOW_E* code for an argument/shape error (nothing
 *     launched), or a positive hipError_t if the launch failed;
 *   - is stateless and re-entrant (one process per GPU is the intended deployment).
 * The caller owns every buffer.  Tensors are contiguous unless a stride argument says otherwise.
 *
 * Reference interfaces replaced (GiaKhangLuu/SCFlow, /root/reference):
 *   scflow_corr_pyramid      <- CorrelationPyramid.forward      models/decoder/raft_decoder.py:35-58
 *   scflow_corr_lookup       <- CorrLookup.forward              models/utils/corr_lookup.py:102-136
 *   scflow_conv2d (+ GRU epilogues) <- ConvGRU.forward          models/decoder/raft_decoder.py:235-253
 *                               and the ConvModule convs of MotionEncoder / XHead / the decoder's
 *                               delta-flow and mask encoders (raft_decoder.py:152-166, 256-294;
 *                               scflow_decoder.py:103-124)
 *   scflow_pose_update       <- get_pose_from_delta_pose (ortho6d, exp)  models/utils/pose.py:124-169
 *   scflow_lift_points       <- cal_3d_2d_corr / lift_2d_to_3d            models/utils/pose.py:26-64
 *   scflow_pose_flow         <- get_flow_from_delta_pose_and_points       models/utils/pose.py:66-88
 *   scflow_pose_update_flow  <- the two calls above fused, as used at     scflow_decoder.py:231-244
 *   scflow_flow_downsample   <- 1/8·F.interpolate(flow, 1/8, bilinear, align_corners=True)  scflow_decoder.py:197-198
 *   scflow_flow_upsample     <- 8·F.interpolate(flow+Δflow, ×8) and mask ×8 (same)          scflow_decoder.py:223-228
 *   scflow_pose_step_call    <- one iteration's tail fused: pose update + pose flow + the ×8
 *                               prediction + the next iteration's ↓8 flow   scflow_decoder.py:197-198, 223-244
 *                               (scflow_pose_step / _part / _heads / _masked: its positional forms)
 *   scflow_convex_upsample   <- RAFT's convex ×8 upsampling of the flow and the occlusion (softmax over
 *                               the 3×3 neighbourhood per sub-pixel)   raft_decoder.py:381-416,
 *                               raft_decoder_mask.py:104-160
 *   scflow_pnp_*             <- BaseFlowRefiner.solve_pose: 2D-3D correspondences + RANSAC-PnP (another
 *                               algorithm than cv2.solvePnPRansac)   base_flow_refiner.py:99-155,
 *                               models/utils/pose.py:182-249
 *   scflow_patch_*           <- ComputeBbox, Crop, Resize, Pad, RemapPose, Normalize: 256² patches and their
 *                               intrinsics from full frames   datasets/pipelines/geometry_transform.py:155-500
 *   scflow_pose_err_sym, scflow_vsd_counts <- bop_toolkit's MSSD / MSPD / VSD pose errors, which the
 *                               reference leaves to that CPU tool after ADD.format_results   metrics/add.py:402-446
 *   scflow_scene_visibility  <- bop_toolkit's calc_gt_masks / calc_gt_info (instance masks, visib_fract,
 *                               boxes), which a ready-made BOP data set ships as files; no reference code
 *   scflow_flow_gt           <- get_flow_from_delta_pose_and_depth + filter_flow_by_mask / _by_depth /
 *                               _by_face_index, one launch   models/utils/pose.py:92-121, models/utils/flow.py:6-59
 *   scflow_flow_epe          <- cal_epe and eval_epe_and_occ's occlusion term   models/utils/flow.py:64-88,
 *                               models/refiner/raft_refiner_flow_mask.py:239-259
 *   scflow_transpose         <- layout plumbing (NCHW <-> channels-last slices), no reference equivalent
 *   scflow_ph_*              <- MultiClassPoseHead.forward                models/head/pose_head.py:201-211
 *   scflow_enc_*             <- RAFTEncoder.forward (Basic; IN / BN)      models/encoder/raft_encoder.py:286-314
 *   scflow_gemm_f32          <- torch.matmul / F.linear in the training step's adjoints (raft_decoder.py:35-58,
 *                               pose_head.py:201-211)
 */
#ifndef SCFLOW_HIP_H
#define SCFLOW_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define SCFLOW_OK 0
#define SCFLOW_EINVAL (-1)      /* null pointer / non-positive size / bad enum */
#define SCFLOW_EUNSUPPORTED (-2) /* valid call, but a shape this build has no kernel for */
#define SCFLOW_EALIGN (-3)      /* pointer or stride not 16-byte aligned where float4 access is used */

#define SCFLOW_ACT_NONE 0
#define SCFLOW_ACT_RELU 1
#define SCFLOW_ACT_SIGMOID 2
#define SCFLOW_ACT_TANH 3

#define SCFLOW_EPI_PLAIN 0  /* out = act(conv + bias) */
#define SCFLOW_EPI_GRU_ZR 1 /* cout = 2·hc: z = σ(.) -> gate[:, :hc];  r = σ(.), rh = r·h -> rh   */
#define SCFLOW_EPI_GRU_Q 2  /* cout = hc:   q = tanh(.);  hid <- (1-z)·hid + z·q  (z from gate)     */

/* pose-update mode word (the depth_transform argument of scflow_pose_update / _update_flow /
 * _step): bit 0 = depth transform (0 'exp', 1 linear); | SCFLOW_POSE_QUAT_XYZW = the delta
 * rotation is a quaternion (x, y, z, w) [n][4] (pose.py:132-133) instead of ortho6d [n][6]. */
#define SCFLOW_POSE_QUAT_XYZW 16

#define SCFLOW_LAYOUT_NCHW 0 /* [N][C][H][W] */
#define SCFLOW_LAYOUT_NHWC 1 /* [N][H][W][stride], channels contiguous */

int scflow_version(void);
const char* scflow_strerror(int code);

/* a1: all-pairs correlation volume and its average-pooled pyramid.
 * f1, f2: [n][c][h][w] (render, real).  pyr: one buffer holding the levels back to back;
 * level l is [n·h·w][h>>l][w>>l] (AvgPool2d(2,2) floors), starting at float offset
 * n·h·w·Σ_{j<l}(h>>j)(w>>j).  level0 = (f1ᵀ f2)/sqrt(c).  num_levels in [1, 8]. */
long long scflow_corr_pyramid_size(int n, int h, int w, int num_levels);
int scflow_corr_pyramid(const float* f1, const float* f2, float* pyr, int n, int c, int h, int w,
                        int num_levels, void* stream);

/* a2: multi-scale (2r+1)² bilinear window lookup, align_corners=True (SCFlow's config), zero padding.
 * flow: [n][2][h][w] (flow_layout NCHW) or [n·h·w][2] (NHWC).  out channel
 * k = lvl·(2r+1)² + a·(2r+1) + b samples x+Δx=a−r, y+Δy=b−r.  out: NCHW [n][L(2r+1)²][h][w]
 * or NHWC with pixel stride out_stride (>= L(2r+1)²). */
int scflow_corr_lookup(const float* pyr, const float* flow, int flow_layout, float* out,
                       int out_layout, int out_stride, int n, int h, int w, int num_levels,
                       int radius, void* stream);
/* The same with grid_sample's align_corners chosen: 1 = the call above; 0 = CorrLookup(align_corners=
 * False) (bilinear_sample's own default, corr_lookup.py:35): sample (g+1)·size/2 − 1/2 after the same
 * g = s·2/max(size−1,1) − 1 normalisation (corr_lookup.py:63-64). */
int scflow_corr_lookup_ex(const float* pyr, const float* flow, int flow_layout, float* out,
                          int out_layout, int out_stride, int n, int h, int w, int num_levels,
                          int radius, int align_corners, void* stream);

/* a1 + a2 with the pyramid in TILED layout: level l of query pixel m is an (h>>l)×(w>>l) map
 * stored in 4×4 tiles of 16 contiguous floats, tiles row-major — element (y, x) at
 * ((y>>2)·((w>>l)>>2) + (x>>2))·16 + (y&3)·4 + (x&3) from the map's start (same map sizes and
 * level offsets as scflow_corr_pyramid).  scflow_corr_pyramid_tiled computes level 0 and pools
 * levels 1..L−1 inside the GEMM epilogue (one launch; values bit-identical to
 * scflow_corr_pyramid's); needs L ≤ 4, h and w multiples of 8 and of 4·2^(L−1), f1/f2 16-B
 * aligned.  scflow_corr_lookup_tiled = scflow_corr_lookup_ex on such a pyramid (same outputs). */
int scflow_corr_pyramid_tiled(const float* f1, const float* f2, float* pyr, int n, int c, int h,
                              int w, int num_levels, void* stream);
int scflow_corr_lookup_tiled(const float* pyr, const float* flow, int flow_layout, float* out,
                             int out_layout, int out_stride, int n, int h, int w, int num_levels,
                             int radius, int align_corners, void* stream);
/* a2 + a3's corr_net.0 fused (inference): out[m][·] = act(W·lookup(pyr, flow)[m] + bias), the
 * lookup of scflow_corr_lookup_tiled (TILED pyramid, num_levels 4, radius 4, h and w multiples of
 * 32) and the 1×1 conv of SCFLOW_CONV_1X1W (weight packed by scflow_conv_pack_weights with bk =
 * SCFLOW_CONV_1X1W, c0 = 324, c1 = 0; cout ≤ 256) in one launch: the correlation features stay
 * in LDS (replaces CorrLookup.forward, corr_lookup.py:102-136, followed by MotionEncoder's first
 * corr_net layer, raft_decoder.py:75-85,152-166).  flow: [n·h·w][2] (NHWC); out: [n·h·w] rows of
 * out_stride floats.  Bit-identical to the two launches it replaces. */
int scflow_corr_lookup_conv1x1(const float* pyr, const float* flow, const float* weight,
                               const float* bias, float* out, int out_stride, int n, int h, int w,
                               int num_levels, int radius, int cout, int act, int align_corners,
                               void* stream);
long long scflow_corr_lookup_conv1x1_lds_bytes(void);
/* Occlusion-masked lookup (the reference's mask_corr, scflow_decoder.py:189-207: corr · mask
 * before the motion encoder): out[m][k] = mask[m] · lookup(pyr, flow)[m][k], mask [n·h·w], for
 * every layout and kernel of scflow_corr_lookup_ex (tiled = 0) / scflow_corr_lookup_tiled (tiled
 * != 0).  The multiply happens where the sample is stored: no extra pass over the L·(2r+1)²
 * features, no extra launch; the result equals (unmasked lookup) · mask bit for bit.  mask NULL:
 * exactly the unmasked call. */
int scflow_corr_lookup_masked(const float* pyr, const float* flow, int flow_layout,
                              const float* mask, float* out, int out_layout, int out_stride, int n,
                              int h, int w, int num_levels, int radius, int align_corners, int tiled,
                              void* stream);
/* scflow_corr_lookup_conv1x1 on the masked lookup: out[m][·] = act(W·(mask[m]·lookup[m]) + bias).
 * The sample is scaled as it enters the LDS A row (the reference's order, conv(corr · mask)), not
 * the accumulator, so the result is bit-identical to scflow_corr_lookup_masked (tiled) followed
 * by the SCFLOW_CONV_1X1W conv.  mask NULL: exactly scflow_corr_lookup_conv1x1. */
int scflow_corr_lookup_conv1x1_masked(const float* pyr, const float* flow, const float* mask,
                                      const float* weight, const float* bias, float* out,
                                      int out_stride, int n, int h, int w, int num_levels,
                                      int radius, int cout, int act, int align_corners,
                                      void* stream);
/* ABI markers: scflow_abi_version() returns SCFLOW_ABI_VERSION of the header the library was
 * built from (2: scflow_conv_args ends with the F(4×4,3×3) workspace fields ws / ws_bytes, and
 * scflow_conv_pick_bk may return SCFLOW_CONV_WINO4; 3: + scflow_xhead_pred and its workspace
 * query; 4: + the occlusion-masked entries scflow_corr_lookup_masked,
 * scflow_corr_lookup_conv1x1_masked, scflow_flow_downsample_masked, scflow_pose_step_masked and
 * scflow_corr_lookup_backward_masked — new exports only); scflow_conv_args_size() its
 * sizeof(scflow_conv_args).  A binding checks both before its first call (scflow_amd/_lib.py
 * does, at load). */
#define SCFLOW_ABI_VERSION 4
int scflow_abi_version(void);
long long scflow_conv_args_size(void);
/* Tuning only: the library's SCFLOW_* environment switches ("Switches") are read
 * once and cached; this makes their next use re-read the environment (in-process A/B). */
int scflow_debug_reload_switches(void);
/* Profiling only: later LDS-kernel lookups (scflow_corr_lookup*) write 6 u64 real-time-clock
 * stamps per workgroup of 16 query pixels to `stamps` (phase boundaries; NULL turns it off). */
int scflow_debug_lookup_stamps(void* stamps);
/* Profiling only: later instrumented conv launches (the Winograd F(2×2,3×3), F(4,5) and F(4×4,3×3)
 * kernels, the bf16 1×5 / 5×1 conv, the small-cin MFMA conv, the whole-halo thin conv,
 * scflow_enc_conv) write 4 u64
 * real-time-clock stamps per workgroup (start, prologue done, main loop done, epilogue done), NULL
 * turns it off. */
int scflow_debug_conv_stamps(void* stamps);

/* Channels-last convolution (cross-correlation, like nn.Conv2d) with fused bias/activation and
 * optional ConvGRU gate epilogues.  Input channels = c0 (src0) ++ c1 (src1, may be 0).
 * Weights must be packed by scflow_conv_pack_weights for the same shape. */
typedef struct scflow_conv_args {
  const float* src0; int c0; int s0;     /* first input, channels, pixel stride (floats)      */
  const float* src1; int c1; int s1;     /* optional second input concatenated on channels     */
  const float* weight;                   /* packed, see scflow_conv_pack_weights               */
  const float* bias;                     /* [cout] or NULL                                     */
  float* out; int so;                    /* output (channel 0 of this conv), pixel stride      */
  int n, h, w;                           /* input batch and spatial size                       */
  int cout, kh, kw, ph, pw, stride;      /* output channels, kernel, padding, stride           */
  int act;                               /* SCFLOW_ACT_*                                       */
  int epilogue;                          /* SCFLOW_EPI_*                                       */
  float* gate; int sg;                   /* GRU z buffer and its pixel stride                  */
  float* rh; int srh;                    /* GRU_ZR: r·h output                                 */
  float* hid; int sh;                    /* GRU: hidden state (read by ZR, updated by Q)       */
  const float* bias_map; int sbm;        /* optional per-pixel additive term [pix][sbm] (MFMA  */
                                         /* variant): pre-activation += bias_map[pix·sbm + o]; */
                                         /* the decoder passes the loop-invariant context      */
                                         /* contribution of the GRU convs here                 */
  int bk;                                /* packing format of the weights: K-stage depth 0 or 16 */
                                         /* (default) or 8, or SCFLOW_CONV_WINO — see           */
                                         /* scflow_conv_pick_bk                                 */
  /* Winograd 3×3 (SCFLOW_CONV_WINO, _WINO4) and SCFLOW_CONV_BF16_3X3N (NULL elsewhere) — the   */
  /* RAFT encoder's fused normalisation:                                                       */
  const float* in_scale;                 /* src0 ← relu(src0·in_scale[n][c0] + in_shift[n][c0]) */
  const float* in_shift;                 /* on load (InstanceNorm + ReLU of the producer; c1=0) */
  const float* out_scale;                /* v ← (conv + bias)·out_scale[o] + out_shift[o]       */
  const float* out_shift;                /* (eval BatchNorm)                                    */
  const float* res; int sres;            /* v += res[pix·sres + o] before the activation        */
  /* SCFLOW_CONV_WINO4 only (NULL / 0 elsewhere): the transformed-input workspace of at least   */
  /* scflow_conv_workspace_bytes(args) bytes, 16-B aligned, private to this launch until it ends */
  float* ws; long long ws_bytes;
} scflow_conv_args;

/* scflow_conv_args.bk = SCFLOW_CONV_WINO selects the Winograd kernels: F(2×2,3×3) for 3×3, stride
 * 1, pad 1, width 32, 64 or 128 (height a multiple of 4 at 32, of 2 otherwise), SCFLOW_EPI_PLAIN;
 * F(4,5) for 1×5 (pad 0,2) / 5×1 (pad 2,0), width 32 or 64, every epilogue.  Exact fp32
 * arithmetic, 2.25× / 2.5× fewer matrix multiplies than the direct conv; the weights must be
 * packed with the same bk. */
#define SCFLOW_CONV_WINO 2
/* scflow_conv_args.bk = SCFLOW_CONV_1X1W selects the wide 1×1 kernel (corr_net.0's 324 → 256):
 * stride 1, no padding, one source (c1 = 0) with c0 a multiple of 4 and 8·⌈c0/8⌉ one of the
 * instantiated depths (128, 256, 328), cout ≤ 256, SCFLOW_EPI_PLAIN (bias, bias map, activation);
 * 64 pixels × every output channel per workgroup, the pixels' whole input rows in LDS. */
#define SCFLOW_CONV_1X1W 3
/* scflow_conv_args.bk = SCFLOW_CONV_WINO4 selects Winograd F(4×4,3×3) (round 5): 3×3, stride 1,
 * pad 1, height and width multiples of 4, channels multiples of 4, SCFLOW_EPI_PLAIN (bias, bias
 * map, residual, eval-BN affine, input IN+ReLU on load with c1 = 0, activation); 2.25 multiplies
 * per output and tap set (F(2×2,3×3): 4).  Two launches: the input transform into args.ws, then
 * the 36 point GEMMs with the output transform in their epilogue.  fp32 throughout; error vs fp64
 * ≈ 10× a direct fp32 conv's (points {0, ±1, 2, −½, ∞}). */
#define SCFLOW_CONV_WINO4 4
/* scflow_conv_args.bk = SCFLOW_CONV_BF16 selects the bf16 direct conv for the SeqConv GRU (opt-in:
 * scflow_conv_pick_bk never returns it): 1×5 (pad 0,2) / 5×1 (pad 2,0), stride 1, width 32 or 64,
 * the height conditions of F(4,5), c0 and c1 multiples of 32 (c1 may be 0), cout a multiple of 32,
 * every epilogue, no fused normalisation or residual; anything else is SCFLOW_EUNSUPPORTED.
 * Inputs are rounded to bf16 (nearest even) on their way into LDS and the weights when packed;
 * products are exact and accumulate in fp32 on v_mfma_f32_32x32x16_bf16; bias, bias map,
 * activation and the GRU epilogues are fp32 and every buffer stays fp32.  No workspace.  Packed
 * size in floats (two bf16 per float): 64·⌈cout/64⌉ · (c0 + c1) · 5 / 2.  (5 is not a format.) */
#define SCFLOW_CONV_BF16 6
/* scflow_conv_args.bk = SCFLOW_CONV_BF16_3X3 selects the bf16 direct 3×3 conv for the motion
 * encoder (opt-in: scflow_conv_pick_bk never returns it; SCFLOW_CONV_BF16 keeps refusing 3×3):
 * 3×3, pad (1,1), stride 1, width 32 or 64, height a multiple of 4, c0 and c1 multiples of 32
 * (c1 may be 0), any cout ≥ 1 (stores are masked per channel: nothing at or past cout of the
 * output's pixel stride is written), the plain epilogue only — no GRU epilogue, bias map, fused
 * normalisation or residual; anything else is SCFLOW_EUNSUPPORTED.  Inputs are rounded to bf16
 * (nearest even) on their way into LDS and the weights when packed; products are exact and
 * accumulate in fp32 on v_mfma_f32_32x32x16_bf16; bias and activation are fp32 and every buffer
 * stays fp32.  No workspace.  Packed size in floats (two bf16 per float):
 * 32·⌈cout/32⌉ · (c0 + c1) · 9 / 2. */
#define SCFLOW_CONV_BF16_3X3 7
/* scflow_conv_args.bk = SCFLOW_CONV_BF16_3X3N selects the same kernel in the RAFT encoder's form
 * (opt-in: scflow_conv_pick_bk never returns it; SCFLOW_CONV_BF16_3X3 keeps its own domain): 3×3,
 * pad (1,1), stride 1, width any multiple of 32, height a multiple of 4, c0 and c1 multiples of 32
 * (c1 may be 0), any cout ≥ 1, the plain epilogue without bias map; anything else is
 * SCFLOW_EUNSUPPORTED.  Fused, each optional: x' = relu(fmaf(x, in_scale[img][c], in_shift[img][c]))
 * on load (one fp32 rounding, then the bf16 rounding; needs both pointers and c1 = 0; zero padding
 * stays 0); v = conv + bias; v = v·out_scale[o] + out_shift[o]; v += res[pix·sres + o]; out =
 * act(v).  in_scale without in_shift, out_scale without out_shift (or the reverse) and sres < cout
 * are SCFLOW_EINVAL; a source pixel stride or sres that is not a multiple of 4 floats, or an
 * in_scale / in_shift that is not 16-byte aligned, is SCFLOW_EALIGN.  With every fused pointer NULL
 * a launch equals SCFLOW_CONV_BF16_3X3's bit for bit.  Packing and packed size are
 * SCFLOW_CONV_BF16_3X3's; no workspace, no atomics, a fixed summation order. */
#define SCFLOW_CONV_BF16_3X3N 9
/* Two independent convolutions (neither reads what the other writes, no overlapping outputs) in
 * ONE grouped launch when a paired kernel covers the pair — the decoder tail's flow-predictor /
 * mask-predictor branches: 3×3 256→2 with 1×1 256→1, 7×7 2→128 with 3×3 1→64, two F(2×2,3×3)
 * convs of one width — else as two scflow_conv2d launches in order; results equal the separate
 * launches bit for bit (round 6; replaces running the two branches on two streams joined by
 * events, scflow_decoder.py:211-218). */
int scflow_conv2d_pair(const scflow_conv_args* args_a, const scflow_conv_args* args_b, void* stream);
/* The XHeads (raft_decoder.py:256-294, called at scflow_decoder.py:211-218): the two hidden 3×3
 * convs as ONE F(4×4,3×3) conv `hidden` (SCFLOW_CONV_WINO4, flow head's channels first —
 * flow_channels of hidden->cout —, ReLU, bias only; hidden->out is not written) with both
 * predictors contracted in its epilogue, then one launch summing the 32-channel blocks' partial
 * sums and the 3×3 predictor's taps (round 6; replaces the hidden conv's 2 KiB-per-pixel output
 * and the predictor convs that read it back).  pred_w [hidden->cout][20]: row c < flow_channels
 * holds the 3×3 two-output predictor's weights W[o][c][ty][tx] at column (3·ty + tx)·2 + o (18
 * used), row c ≥ flow_channels the 1×1 one-output predictor's W[0][c − flow_channels] at column 0.
 * flow_out [pixel][flow_stride] (2 channels) = flow_act(flow_bias + conv), mask_out
 * [pixel][mask_stride] = mask_act(mask_bias + conv) (biases may be NULL).  workspace ≥
 * scflow_xhead_pred_workspace_bytes, 16-byte aligned.  Width 32 or 64, height a multiple of 4,
 * both heads' hidden channels multiples of 32; else SCFLOW_EUNSUPPORTED.  fp32; only the
 * summation order differs from the separate convs. */
long long scflow_xhead_pred_workspace_bytes(int n, int h, int w, int flow_channels, int hidden_channels);
int scflow_xhead_pred(const scflow_conv_args* hidden, int flow_channels, const float* pred_w,
                      float* workspace, long long workspace_bytes, const float* flow_bias,
                      const float* mask_bias, int flow_act, int mask_act, float* flow_out,
                      int flow_stride, float* mask_out, int mask_stride, void* stream);
/* Bytes of args.ws a launch needs (0 for packing formats without a workspace). */
long long scflow_conv_workspace_bytes(const scflow_conv_args* args);

/* Number of floats of the packed weight buffer for bk 8 and 16 (the same for both); w_oihw is
 * nn.Conv2d's [cout][c0+c1][kh][kw]. */
long long scflow_conv_packed_size(int cout, int c0, int c1, int kh, int kw, int stride, int w);
/* The same for any packing format bk (0, 8, 16, SCFLOW_CONV_WINO, SCFLOW_CONV_1X1W,
 * SCFLOW_CONV_WINO4, SCFLOW_CONV_BF16, SCFLOW_CONV_BF16_3X3 or SCFLOW_CONV_BF16_3X3N). */
long long scflow_conv_packed_size_bk(int cout, int c0, int c1, int kh, int kw, int stride, int w,
                                     int bk);
/* bk: packing format (0 → 16, 8, SCFLOW_CONV_WINO or SCFLOW_CONV_1X1W); pass the same value in
 * scflow_conv_args.bk. */
int scflow_conv_pack_weights(const float* w_oihw, float* packed, int cout, int c0, int c1, int kh,
                             int kw, int stride, int w, int bk, void* stream);
/* Preferred packing format for this launch shape (batch, sizes, channels, kernel): Winograd
 * (SCFLOW_CONV_WINO) for the 3×3 stride-1 convs it covers, the wide 1×1 kernel
 * (SCFLOW_CONV_1X1W) for the 1×1 convs it covers, else the direct conv's K-stage depth,
 * 8 when the grid needs more resident workgroups than 16-deep stages' LDS allows, else 16. */
int scflow_conv_pick_bk(const scflow_conv_args* args);
int scflow_conv2d(const scflow_conv_args* args, void* stream);
/* Host-only query of the launch plan (no launch, no device access, src / weight / out are never
 * dereferenced).  b NULL: *kind = the kernel family scflow_conv2d launches for a (SCFLOW_PLAN_*,
 * SCFLOW_PLAN_NONE if refused); returns the status scflow_conv2d answers before launching.
 * b non-NULL: *kind = the grouped kernel scflow_conv2d_pair launches for the two in either order
 * (SCFLOW_PAIR_*, SCFLOW_PAIR_NONE: two launches); returns the status scflow_conv2d_pair answers
 * before launching (an invalid half refuses the pair). */
int scflow_conv_plan_kind(const scflow_conv_args* a, const scflow_conv_args* b, int* kind);
#define SCFLOW_PLAN_NONE 0
#define SCFLOW_PLAN_MFMA 1              /* direct implicit-GEMM conv (conv_mfma_kernel)          */
#define SCFLOW_PLAN_1X1 2               /* conv1x1_kernel: 1×1 on 128-pixel tiles                */
#define SCFLOW_PLAN_1X1W 3              /* wide 1×1 (SCFLOW_CONV_1X1W)                           */
#define SCFLOW_PLAN_WINO 4              /* Winograd F(2×2,3×3)                                   */
#define SCFLOW_PLAN_WINO5 5             /* Winograd F(4,5), 1×5 / 5×1                            */
#define SCFLOW_PLAN_WINO4 6             /* Winograd F(4×4,3×3): transform + GEMM launches        */
#define SCFLOW_PLAN_SMALLCIN_MFMA 7     /* cin ≤ 2 on MFMA, whole rows of 32 / 64 pixels         */
#define SCFLOW_PLAN_SMALLCIN_TILED 8    /* cin ≤ 2, one lane per output channel, 32-pixel tiles  */
#define SCFLOW_PLAN_SMALLCIN_GENERIC 9  /* cin ≤ 4, any shape                                    */
#define SCFLOW_PLAN_THINZ 10            /* cout ≤ 2: 3×3 256-channel contraction on MFMA         */
#define SCFLOW_PLAN_THIN_FULL 11        /* cout ≤ 2: 3×3, the whole halo in LDS                  */
#define SCFLOW_PLAN_THIN_CHUNKED 12     /* cout ≤ 2: halo in 32-channel chunks                   */
#define SCFLOW_PLAN_THIN_GENERIC 13     /* cout ≤ 4, any shape                                   */
#define SCFLOW_PLAN_SEP_BF16 14         /* bf16 direct 1×5 / 5×1 (SCFLOW_CONV_BF16)              */
#define SCFLOW_PLAN_C3_BF16 15          /* bf16 direct 3×3 (SCFLOW_CONV_BF16_3X3)                */
#define SCFLOW_PLAN_C3_BF16N 16         /* its RAFT-encoder form (SCFLOW_CONV_BF16_3X3N)         */
#define SCFLOW_PAIR_NONE 0
#define SCFLOW_PAIR_THIN 1              /* THINZ (cout 2) beside THIN_CHUNKED 1×1 (cout 1)       */
#define SCFLOW_PAIR_SMALLCIN 2          /* SMALLCIN_MFMA 7×7 2→128 beside 3×3 1→64               */
#define SCFLOW_PAIR_WINO 3              /* two WINO convs of one width (32 or 64)                */

/* a8: R_dst = R(ortho6d Δ)·R_src; t_z' = t_z/exp(Δt_z) (depth_transform 0) or t_z·(Δt_z+1) (1);
 * t_xy' = t_z'·(Δt_xy/weight + t_xy/t_z).  drot6 [n][6], dt [n][3], R [n][3][3], t [n][3]. */
int scflow_pose_update(const float* drot6, const float* dt, const float* R_src, const float* t_src,
                       float* R_dst, float* t_dst, int n, float weight, int depth_transform,
                       void* stream);

/* a9: object-frame point of every pixel: points[n][y][x] = {R⁻¹(K⁻¹[x·d,y·d,d] − t), valid},
 * valid = (depth>0) ? 1 : 0, float4 per pixel. */
int scflow_lift_points(const float* depth, const float* K, const float* R, const float* t,
                       float* points, int n, int h, int w, void* stream);

/* a10: flow[n][2][h][w] = proj(K(R·P+t)) − (x,y) where valid, else invalid_num. */
int scflow_pose_flow(const float* R, const float* t, const float* K, const float* points,
                     float* flow, int n, int h, int w, float invalid_num, void* stream);

/* a8+a10 fused (one launch per refinement iteration). */
int scflow_pose_update_flow(const float* drot6, const float* dt, const float* R_src,
                            const float* t_src, const float* K, const float* points, float* R_dst,
                            float* t_dst, float* flow, int n, int h, int w, float weight,
                            int depth_transform, float invalid_num, void* stream);

/* a11 down: out = value_scale · bilinear(flow[n][2][H][W] -> h×w, align_corners=True) written
 * channels-last to out0 (pixel stride s0) and, if out1 != NULL, also to out1 (stride s1). */
int scflow_flow_downsample(const float* flow, float* out0, int s0, float* out1, int s1, int n,
                           int H, int W, int h, int w, float value_scale, void* stream);
/* ... under the reference's mask_flow (scflow_decoder.py:189-207: the flow entering the motion
 * encoder is flow · mask): out0 keeps the unmasked ↓8 flow (the lookup's centroids), out1 and
 * outm (stride sm; either may be NULL) receive it times mask[n·h·w].  mask NULL: × 1. */
int scflow_flow_downsample_masked(const float* flow, float* out0, int s0, float* out1, int s1,
                                  const float* mask, float* outm, int sm, int n, int H, int W,
                                  int h, int w, float value_scale, void* stream);

/* a11 up: flow_out[n][2][H][W] = value_scale·bilinear(lr + delta) and mask_out[n][1][H][W] =
 * bilinear(mask); lr/delta are channels-last [n·h·w][2] (delta may be NULL), mask [n·h·w][1]
 * (may be NULL, then mask_out is not written). */
int scflow_flow_upsample(const float* lr, const float* delta, const float* mask, float* flow_out,
                         float* mask_out, int n, int h, int w, int H, int W, float value_scale,
                         void* stream);

/* RAFT's convex upsampling (RAFTDecoder._upsample, raft_decoder.py:381-416; RAFTDecoderMask.
 * upsample_flow / upsample_mask, raft_decoder_mask.py:104-160), one launch.  With s = scale = 8 and
 * k = ky·3 + kx over the 3×3 neighbourhood (grid_side = 3):
 *   w[k][sy][sx]                 = softmax over k of logit_scale · logits[pixel][k·64 + sy·8 + sx]
 *   flow_up[n][c][8y+sy][8x+sx]  = value_scale · Σ_k w[k][sy][sx] · (lr + delta)[n][y+ky-1][x+kx-1][c]
 *   occ_up [n][0][8y+sy][8x+sx]  =               Σ_k w[k][sy][sx] ·  occ        [n][y+ky-1][x+kx-1]
 * Neighbours outside the map count as zero (F.unfold(padding=1)) and are never loaded.  One softmax
 * (maximum subtracted) serves both outputs.  logits: channels-last [n·h·w][≥ 576] with pixel stride
 * ls; lr, delta (may be NULL): channels-last [n·h·w][2]; occ (may be NULL, then occ_up is not
 * written): [n·h·w][1].  flow_up [n][2][8h][8w] and occ_up [n][1][8h][8w] are NCHW and 16-byte
 * aligned (float4 stores along the rows; else SCFLOW_EALIGN).  next0 / next1 (either may be NULL;
 * pixel strides s0 / s1 ≥ 2) receive lr + delta channels-last, the next iteration's flow — as
 * out0 / out1 of scflow_flow_downsample; they must not alias lr or delta (a workgroup reads its
 * neighbours' pixels).  scale ≠ 8 or grid_side ≠ 3: SCFLOW_EUNSUPPORTED. */
int scflow_convex_upsample(const float* logits, int ls, const float* lr, const float* delta,
                           const float* occ, float* flow_up, float* occ_up, float* next0, int s0,
                           float* next1, int s1, int n, int h, int w, int scale, int grid_side,
                           float logit_scale, float value_scale, void* stream);

/* The adjoint of scflow_convex_upsample (training).  With the notation above, v_c = x channel c
 * (vs_c = value_scale) or occ (vs_c = 1), g_c[p][s] the incoming gradient at output pixel
 * (8y+sy, 8x+sx) of channel c and nb(p, k) = p + (ky-1, kx-1):
 *   dw[k][s]                     = Σ_c vs_c · v_c[nb(p,k)] · g_c[p][s]      (out-of-map: 0)
 *   dlogits[pixel][k·64 + s]     = logit_scale · w[k][s] · (dw[k][s] − Σ_j w[j][s] · dw[j][s])
 *   dx[q][c], docc[q]            = vs_c · Σ_k Σ_s w[k][s] · g_c[p][s] over the in-map p with nb(p,k) = q
 * The softmax is recomputed from the logits as the forward computes it; nothing is kept between
 * the two.  No float atomics and a fixed summation order: the result is bitwise reproducible.
 * logits [n·h·w][≥ 576] (pixel stride ls), x [n·h·w][2] (the flow that was upsampled, lr + delta),
 * occ [n·h·w] or NULL; g_flow [n][2][8h][8w], g_occ [n][1][8h][8w] or NULL (also with occ given:
 * its term is zero), both 16-byte aligned (else SCFLOW_EALIGN).  Outputs: dlogits [n·h·w][≥ 576]
 * with pixel stride dls (channels 0..575 written, nothing else), dx [n·h·w][2], docc [n·h·w] or
 * NULL (zeros when g_occ is NULL).  g_occ or docc without occ: SCFLOW_EINVAL.  ws: a workspace of
 * at least n·h·w · 9 · C floats (C = 3 with occ and g_occ, else 2; 108·n·h·w bytes always do),
 * ws_bytes its size; it holds the per-pixel partial sums between the two launches.  scale ≠ 8 or
 * grid_side ≠ 3: SCFLOW_EUNSUPPORTED.  An error launches nothing. */
int scflow_convex_upsample_bwd(const float* logits, int ls, const float* x, const float* occ,
                               const float* g_flow, const float* g_occ, float* dlogits, int dls,
                               float* dx, float* docc, void* ws, long long ws_bytes, int n, int h,
                               int w, int scale, int grid_side, float logit_scale,
                               float value_scale, void* stream);

/* The RAFT decoders' bilinear branch (convex_unsample_flow=False) has no launch that produces the
 * next iteration's flow: out0 (pixel stride s0) and, if not NULL, out1 (stride s1) = lr + delta,
 * all channels-last [n·h·w][2].  out0 / out1 must not alias lr or delta. */
int scflow_flow_add(const float* lr, const float* delta, float* out0, int s0, float* out1, int s1,
                    int n, int h, int w, void* stream);

/* One launch = scflow_pose_update_flow(drot6 .. invalid_num; flow is [n][2][H][W]) +
 * scflow_flow_upsample(lr, delta, mask, flow_up, mask_up, n, h, w, H, W, up_scale) when flow_up
 * != NULL + scflow_flow_downsample(flow, lr_next, s_next, hx_next, s_hx, n, H, W, h, w,
 * down_scale) when lr_next != NULL (the ↓8 flow is computed from the new pose directly, bit-
 * identical to downsampling `flow`).  lr_next must not alias lr.  A positional form of
 * scflow_pose_step_call (below): parts = 3, no heads, no masked tail; drot6 NULL is refused. */
int scflow_pose_step(const float* drot6, const float* dt, const float* R_src, const float* t_src,
                     const float* K, const float* points, float* R_dst, float* t_dst, float* flow,
                     int n, int H, int W, float weight, int depth_transform, float invalid_num,
                     const float* lr, const float* delta, const float* mask, float* flow_up,
                     float* mask_up, float* lr_next, int s_next, float* hx_next, int s_hx, int h,
                     int w, float up_scale, float down_scale, void* stream);

/* Cross-stream ordering on one device (the decoder's side stream): events without timing and
 * with a device-scope release (hipEventDisableSystemFence) — a default event's system-scope
 * release writes back the GPU caches on every record.  No reference equivalent (plumbing). */
int scflow_sync_event_create(void** event);
int scflow_sync_event_destroy(void* event);
int scflow_sync_event_record(void* event, void* stream);
int scflow_stream_wait_event(void* stream, void* event);
/* Timing events (device-scope release; destroy with scflow_sync_event_destroy, record with
 * scflow_sync_event_record); *ms = end − start after waiting for end. */
int scflow_timing_event_create(void** event);
int scflow_event_elapsed_ms(void* start, void* end, float* ms);

/* out[n·ons + b·obs + a] = in[n·ins + a·ias + b] for a < A, b < B (batched 2-D transpose; e.g.
 * NCHW -> a channel slice of an NHWC buffer, or back). */
int scflow_transpose(const float* in, float* out, int n, int A, int B, long long ins, int ias,
                     long long ons, int obs, void* stream);

/* a7: MultiClassPoseHead (pose_head.py:110-211) as 9 launches.
 * scflow_ph_conv: x (two channel sources, channels-last, pixel strides s0/s1) → raw conv output
 *   out [n][oh][ow][cout] (channels-last, + bias if given).  If scale/shift are given, the input
 *   is first mapped x ← relu(x·scale[n][c] + shift[n][c]) (the previous GroupNorm + ReLU).
 *   Weights packed by scflow_ph_conv_pack ([cout][kh·kw][roundup(cin,16)]).
 * scflow_ph_gn_stats: GroupNorm(groups) statistics of x [n][hw][c] → scale/shift [n][c] with
 *   scale = γ/sqrt(var+eps), shift = β − mean·scale (biased variance, like F.group_norm).
 * scflow_ph_fc: y [m][n] = act(x [m][k] · Wᵀ + b), W = nn.Linear weight [n][k] (k % 16 == 0).
 *   gn_c > 0: x is a raw conv output [m][hw][gn_c] (channels-last) mapped through scale/shift +
 *   ReLU; W's columns must then be in channels-last order — scflow_ph_fc_permute turns the
 *   reference's NCHW-flatten columns (k = c·hw + p, nn.Flatten) into that order.
 * scflow_ph_heads: drot [m][rch] and dt [m][3] from x [m][k] using only class label[0]'s rows of
 *   the rotation [num_class·rch][k] and translation [num_class·3][k] heads (index_select quirk). */
long long scflow_ph_conv_packed_size(int cout, int cin, int kh, int kw);
int scflow_ph_conv_pack(const float* w_oihw, float* packed, int cout, int cin, int kh, int kw,
                        void* stream);
int scflow_ph_conv(const float* src0, int c0, int s0, const float* src1, int c1, int s1,
                   const float* scale, const float* shift, const float* packed, const float* bias,
                   float* out, int n, int h, int w, int cout, int kh, int kw, int stride, int pad,
                   void* stream);
/* scflow_ph_conv with the K chunks split over ksplit workgroup slices: out = ksplit partial slabs
 *   [ksplit][n·oh·ow][cout] (bias must be NULL), summed by scflow_ph_gn_reduce. */
int scflow_ph_conv_split(const float* src0, int c0, int s0, const float* src1, int c1, int s1,
                         const float* scale, const float* shift, const float* packed,
                         const float* bias, float* out, int n, int h, int w, int cout, int kh,
                         int kw, int stride, int pad, int ksplit, void* stream);
int scflow_ph_gn_stats(const float* x, int n, int hw, int c, int groups, const float* gamma,
                       const float* beta, float eps, float* scale, float* shift, void* stream);
/* scflow_ph_gn_reduce: y = Σ_z parts[z] (nsplit slabs, split_stride floats apart; y written when
 *   nsplit > 1) and its GroupNorm scale/shift like scflow_ph_gn_stats (c % 32 == 0). */
int scflow_ph_gn_reduce(const float* parts, int nsplit, long long split_stride, float* y, int n,
                        int hw, int c, int groups, const float* gamma, const float* beta, float eps,
                        float* scale, float* shift, void* stream);
int scflow_ph_fc_permute(const float* W, float* Wp, int n, int c, int hw, void* stream);
int scflow_ph_fc(const float* x, int ldx, int m, int k, const float* W, const float* bias, float* y,
                 int n, int relu, int gn_c, const float* scale, const float* shift, void* stream);
/* scflow_ph_fc with K split over ksplit workgroup slices (m ≤ 32): parts [ksplit][m][n] = partial
 *   x·Wᵀ sums (no bias / activation); gn_c/scale/shift as in scflow_ph_fc, or xsplit > 0: x is
 *   the previous layer's split partial sums [xsplit][m][ldx] read as relu(Σ + xbias).
 * scflow_ph_fc_sum: y [m][n] = act(x' · Wᵀ + b) with x' = relu(Σ_z parts[z] + xbias), the input
 *   being the previous layer's split partial sums [nsplit][m][k] (its bias xbias, then ReLU).
 * scflow_ph_heads_sum: scflow_ph_heads on such a split input (xsplit = 0: plain x). */
int scflow_ph_fc_split(const float* x, int ldx, int m, int k, const float* W, float* parts, int n,
                       int ksplit, int gn_c, const float* scale, const float* shift, int xsplit,
                       const float* xbias, void* stream);
int scflow_ph_fc_sum(const float* parts, int nsplit, int m, int k, const float* xbias,
                     const float* W, const float* bias, float* y, int n, int relu, void* stream);
int scflow_ph_heads_sum(const float* x, int xsplit, const float* xbias, int m, int k,
                        const float* Wr, const float* br, int rch, const float* Wt, const float* bt,
                        const long long* label, int num_class, float* drot, float* dt,
                        void* stream);
int scflow_ph_heads(const float* x, int m, int k, const float* Wr, const float* br, int rch,
                    const float* Wt, const float* bt, const long long* label, int num_class,
                    float* drot, float* dt, void* stream);

/* scflow_pose_step_part: scflow_pose_step restricted to parts (bit 0: the full-resolution outputs
 *   — pose flow, ×8 flow prediction and mask; bit 1: the next iteration's ↓8 flow, lr_next /
 *   hx_next).  Each part recomputes the pose update; the part with the lowest block writes
 *   R_dst / t_dst.  The decoder runs bit 1 on its critical path and bit 0 on a side stream.
 *   drot6 == NULL (parts = 1 only): R_src / t_src ARE the updated pose (the bit-1 launch's
 *   R_dst / t_dst) — no update, dt / R_dst / t_dst unused, same outputs.  A positional form of
 *   scflow_pose_step_call: no heads, no masked tail. */
int scflow_pose_step_part(const float* drot6, const float* dt, const float* R_src,
                          const float* t_src, const float* K, const float* points, float* R_dst,
                          float* t_dst, float* flow, int n, int H, int W, float weight,
                          int depth_transform, float invalid_num, const float* lr,
                          const float* delta, const float* mask, float* flow_up, float* mask_up,
                          float* lr_next, int s_next, float* hx_next, int s_hx, int h, int w,
                          float up_scale, float down_scale, int parts, void* stream);

/* scflow_pose_step_heads: scflow_pose_step_part with the pose head's rotation / translation heads
 *   (MultiClassPoseHead, models/head/pose_head.py:203-211 — label[0]'s class for every sample)
 *   computed in the same launch instead of by scflow_ph_heads_sum: x = relu(Σ_z x_z + xbias),
 *   the last FC's xsplit K-split partial sums [xsplit][n][k]; rch = 6 (ortho6d) or 4
 *   (quaternion, depth_transform's SCFLOW_POSE_QUAT_XYZW).  drot [n][rch] / dt [n][3] are
 *   OUTPUTS here (the decoder's returned deltas).  Replaces the heads launch + the pose step's
 *   delta reads of the reference's get_pose_ (models/decoder/scflow_decoder.py:230-236).  A
 *   positional form of scflow_pose_step_call: x is required, no masked tail. */
int scflow_pose_step_heads(const float* x, int xsplit, const float* xbias, int k, const float* Wr,
                           const float* br, int rch, const float* Wt, const float* bt,
                           const long long* label, int num_class, float* drot, float* dt,
                           const float* R_src, const float* t_src, const float* K,
                           const float* points, float* R_dst, float* t_dst, float* flow, int n,
                           int H, int W, float weight, int depth_transform, float invalid_num,
                           const float* lr, const float* delta, const float* mask, float* flow_up,
                           float* mask_up, float* lr_next, int s_next, float* hx_next, int s_hx,
                           int h, int w, float up_scale, float down_scale, int parts,
                           void* stream);

/* scflow_pose_step_masked: the superset of scflow_pose_step / _part / _heads with the masked
 *   iteration tail (mask_flow).  x NULL: scflow_pose_step_part's arguments (drot / dt are read);
 *   x != NULL: scflow_pose_step_heads' (drot / dt are written).  mask_next [n·h·w] is the mask
 *   this iteration just predicted: lr_next still receives the unmasked ↓8 flow (the next
 *   lookup's centroids), lrm_next (pixel stride s_lrm; may be NULL; must alias neither lr nor
 *   lr_next) and hx_next receive lr_next · mask_next — the flow branch's input and the motion
 *   features' flow channels of the next iteration.  mask_next NULL: hx_next and lrm_next receive
 *   lr_next, everything as the unmasked entries bit for bit.  The full-resolution outputs never
 *   depend on mask_next.  A positional form of scflow_pose_step_call with every field; drot NULL
 *   is refused even for parts = 1. */
int scflow_pose_step_masked(const float* x, int xsplit, const float* xbias, int k, const float* Wr,
                            const float* br, int rch, const float* Wt, const float* bt,
                            const long long* label, int num_class, float* drot, float* dt,
                            const float* R_src, const float* t_src, const float* K,
                            const float* points, float* R_dst, float* t_dst, float* flow, int n,
                            int H, int W, float weight, int depth_transform, float invalid_num,
                            const float* lr, const float* delta, const float* mask, float* flow_up,
                            float* mask_up, float* lr_next, int s_next, float* hx_next, int s_hx,
                            const float* mask_next, float* lrm_next, int s_lrm, int h, int w,
                            float up_scale, float down_scale, int parts, void* stream);

/* scflow_pose_step_call: the pose step behind one argument struct — the one launcher that the four
 *   positional entries above fill and call.  The fields are scflow_pose_step_masked's parameters
 *   under the same names and meanings.  A zeroed heads block (x NULL), a zeroed masked block
 *   (mask_next / lrm_next NULL) and parts = 3 is scflow_pose_step.  It accepts the union of what
 *   the entries accept: with x NULL what scflow_pose_step_part does (drot NULL with parts = 1 is
 *   the given-pose form; mask_next / lrm_next as in scflow_pose_step_masked), with x != NULL what
 *   scflow_pose_step_masked does. */
typedef struct scflow_pose_step_args {
  /* the fused heads (x NULL: off; drot / dt are then read, else written) */
  const float* x; int xsplit; const float* xbias; int k;
  const float* Wr; const float* br; int rch; const float* Wt; const float* bt;
  const long long* label; int num_class;
  /* the pose update and the pose flow */
  float* drot; float* dt; const float* R_src; const float* t_src; const float* K;
  const float* points; float* R_dst; float* t_dst; float* flow;
  int n, H, W; float weight; int depth_transform; float invalid_num;
  /* the ×8 outputs */
  const float* lr; const float* delta; const float* mask; float* flow_up; float* mask_up;
  int h, w; float up_scale, down_scale;
  /* the next iteration's ↓8 flow */
  float* lr_next; int s_next; float* hx_next; int s_hx;
  /* the masked tail */
  const float* mask_next; float* lrm_next; int s_lrm;
  int parts;                             /* bit 0: full resolution, bit 1: the ↓8 flow */
} scflow_pose_step_args;
int scflow_pose_step_call(const scflow_pose_step_args* args, void* stream);

/* §8(f)-1: RAFTEncoder (Basic) — feature encoder (InstanceNorm) and context encoder (BatchNorm,
 * eval statistics), models/encoder/raft_encoder.py:286-314, BasicBlock models/backbone/resnet.py:
 * 12-92, ResLayer resnet.py:676-771, called from SCFlowRefiner.extract_feat
 * (models/refiner/scflow_refiner.py:84-106).  Activations are channels-last [n][h][w][c].
 *
 * scflow_enc_conv: implicit-GEMM conv (fp32 MFMA), 1×1 or 3×3, stride 1 or 2, cin % 16 == 0;
 *   output width 8, 16, 32, 64 or a multiple of the tile (128 for stride 1, 64 for stride 2), and
 *   output height a multiple of the tile's rows (tile / width when the width is smaller).  Per element of the output:
 *     v = conv(x') + bias;  v = v·out_scale[c] + out_shift[c] (if given: eval BatchNorm);
 *     v += res[pix][c] (if given);  out = act(v) for c < act_split, act2(v) otherwise,
 *   where x' = relu(x·in_scale[img][c] + in_shift[img][c]) if in_scale is given (the previous
 *   InstanceNorm + ReLU applied on load; zero padding stays zero), else x.
 *   Weights packed by scflow_enc_conv_pack (same shape).
 * scflow_enc_stem: 7×7 conv of an NCHW image batch [n][3][h][w], stride 1 or 2 (other shapes:
 *   SCFLOW_EUNSUPPORTED), written channels-last with the same bias / out_scale / act epilogue
 *   (the stem conv1); cout ≤ 64 runs as an implicit GEMM on fp32 MFMA, wider stems on VALU.
 *   Weights packed by scflow_enc_stem_pack ([kh·kw·cin][roundup(cout,64)]).
 *   With src1 the input is cat[src, src1] (both normalised on load when in_scale is given,
 *   in_scale then covering cin + cin1 channels).
 * scflow_enc_stats + scflow_enc_norm_finalize: InstanceNorm statistics of x [n][hw][c]
 *   (fp64 partial sums over `chunks` pixel chunks per image, then per (img, c))
 *   → scale = 1/sqrt(var+eps), shift = −mean·scale (biased variance, affine=False);
 *   partial must hold n·chunks·2·c doubles.
 * scflow_enc_apply: out[p][c] = relu(x·scale[img][c] + shift[img][c] + id'), with
 *   id' = 0 (id NULL), id (id_scale NULL) or id·id_scale[img][c] + id_shift[img][c]. */
typedef struct scflow_enc_conv_args {
  const float* src; int cin; int s_in;            /* input, channels, pixel stride           */
  const float* src1; int cin1; int s_in1;          /* optional 2nd input, concatenated on     */
                                                   /* channels (cin1 % 16 == 0; 0 = none)     */
  int ksplit;                                      /* ≥ 2: K (channel stages) split over      */
                                                   /* grid.z; split z writes a raw partial    */
                                                   /* to out + z·n·oh·ow·s_out (no bias /     */
                                                   /* affine / residual / act allowed)        */
  const float* in_scale; const float* in_shift;    /* [n][cin] or NULL                        */
  const float* weight; const float* bias;          /* packed; bias [cout] or NULL             */
  const float* out_scale; const float* out_shift;  /* [cout] or NULL                          */
  const float* res; int s_res;                     /* residual or NULL, pixel stride          */
  float* out; int s_out;                           /* output, pixel stride                    */
  int n, h, w, cout, kh, kw, stride, pad;
  int act, act2, act_split;                        /* SCFLOW_ACT_* and the channel split      */
} scflow_enc_conv_args;

long long scflow_enc_conv_packed_size(int cout, int cin, int kh, int kw);
int scflow_enc_conv_pack(const float* w_oihw, float* packed, int cout, int cin, int kh, int kw,
                         void* stream);
int scflow_enc_conv(const scflow_enc_conv_args* args, void* stream);
long long scflow_enc_stem_packed_size(int cout, int cin, int kh, int kw);
int scflow_enc_stem_pack(const float* w_oihw, float* packed, int cout, int cin, int kh, int kw,
                         void* stream);
int scflow_enc_stem(const float* img, const float* packed, const float* bias,
                    const float* out_scale, const float* out_shift, float* out, int n, int cin,
                    int h, int w, int cout, int kh, int kw, int stride, int pad, int act,
                    void* stream);
int scflow_enc_stats(const float* x, int n, int hw, int c, int chunks, double* partial,
                     void* stream);
int scflow_enc_norm_finalize(const double* partial, int n, int chunks, int c, int hw, float eps,
                             float* scale, float* shift, void* stream);
int scflow_enc_apply(const float* x, const float* scale, const float* shift, const float* id,
                     const float* id_scale, const float* id_shift, float* out, int n, int hw,
                     int c, void* stream);

/* Training (§8(f)-2) building blocks.
 * scflow_im2col: cols[p][(ty·kw + tx)·cin + c] = x[n][oy·s − ph + ty][ox·s − pw + tx][c] (0 outside),
 *   p = (n·oh + oy)·ow + ox; x channels-last with pixel stride sx.  The conv weight gradient is
 *   then dW[o][tap·cin + c] = Σ_p dY[p][o] · cols[p][tap·cin + c] (a plain GEMM).
 * scflow_corr_lookup_backward: scatter-add of the lookup's output gradient (same layout options
 *   as scflow_corr_lookup) into the pyramid gradient (same layout as the pyramid; must be
 *   zeroed by the caller), with grid_sample's bilinear weights — the flow input is detached in
 *   SCFlow (scflow_decoder.py:193-194), so no flow gradient. */
int scflow_im2col(const float* x, int sx, float* cols, int n, int h, int w, int cin, int kh, int kw,
                  int stride, int ph, int pw, void* stream);
/* scflow_im2col_ex: scflow_im2col, or with channel_major the column order (c·kh + ty)·kw + tx —
 * the conv weight's own [cout][cin][kh][kw] order, so dW (and its accumulation) is one GEMM
 * written in place. */
int scflow_im2col_ex(const float* x, int sx, float* cols, int n, int h, int w, int cin, int kh,
                     int kw, int stride, int ph, int pw, int channel_major, void* stream);
/* scflow_pose_update6_train: the training step's pose update for an ortho6d Δrotation
 * (pose.py:124-169), forward (backward = 0: o0 = Rn [n][3][3], o1 = tn [n][3]) or its gradient
 * (backward = 1, given gRn, gtn: o0 = g drot [n][6], o1 = g dt [n][3], o2 = g R, o3 = g t);
 * depth_exp: depth_transform 'exp' (else 'linear'); detach_xy: detach_depth_for_xy. */
int scflow_pose_update6_train(const float* drot, const float* dt, const float* R, const float* t,
                              const float* gRn, const float* gtn, float* o0, float* o1, float* o2,
                              float* o3, int n, float weight, int depth_exp, int detach_xy,
                              int backward, void* stream);
/* scflow_pm_loss / scflow_pm_loss_backward: one refinement iteration's disentangled L1
 * point-matching loss (point_matching_loss.py:159-218, disentangle_z, mean) fused — model points
 * pts [B][P][3] (each sample's class's set), rotations [B][3][3], translations [B][3], sym [B]
 * (1.0 = symmetric class: nearest-point matching as scflow_knn1; NULL = none), diam [B];
 * workspace gt_rt, pred_rot [B][P][3], idx [B][P]; loss = weight·Σ_b l_b/diam_b/B (one float).
 * The backward takes the loss gradient (one float, device) and the forward's workspace and
 * writes g_pred_r [B][3][3], g_pred_t [B][3]. */
int scflow_pm_loss(const float* pts, const float* gt_r, const float* gt_t, const float* pred_r,
                   const float* pred_t, const float* sym, const float* diam, float* gt_rt,
                   float* pred_rot, long long* idx, float* loss, int B, int P, float weight,
                   void* stream);
int scflow_pm_loss_backward(const float* gloss, const float* pts, const float* gt_rt,
                            const float* pred_rot, const long long* idx, const float* sym,
                            const float* pred_t, const float* gt_t, const float* diam,
                            float* g_pred_r, float* g_pred_t, int B, int P, float weight,
                            void* stream);
/* scflow_up_l1_loss: a full-resolution L1 loss of the sequence loss on the ×(H/h) bilinear
 * (align_corners) upsampling of the channels-last low-resolution prediction f [N][h][w][C]:
 * loss = weight·Σ v·|sval·up(f) − target| / denom (target NCHW [N][C][H][W], v = vmask [N][H][W]
 * or 1, denom = *denom (device) or cdenom), RAFTLoss / L1Loss of sequence_loss.py:15-36 after
 * scflow_decoder.py:223-228.  Writes sgn = v·sgn(sval·up − target) [N][C][H][W] for the backward
 * (the upsampling adjoint) and uses partial[ceil(N·H·W/256)] as workspace. */
int scflow_up_l1_loss(const float* f, int C, int h, int w, const float* target, const float* vmask,
                      int N, int H, int W, float sval, const float* denom, float cdenom,
                      float weight, float* sgn, float* partial, float* loss, void* stream);
/* scflow_knn1: idx[b][i] = argmin_j |gt[b][i] − pred[b][j]|² over [batch][P][3] / [batch][Q][3]
 * point sets (first minimum in index order) — pytorch3d knn_points(K=1) in the symmetric-class
 * point-matching loss (point_matching_loss.py:183-186; pytorch3d is absent, torch.argmin's rule). */
int scflow_knn1(const float* gt, const float* pred, long long* idx, int batch, int P, int Q,
                void* stream);
/* GroupNorm (+ReLU) of the pose head's conv stack (pose_head.py:160-170, mmcv ConvModule with
 * norm_cfg GN(32) and ReLU; torch.nn.GroupNorm semantics: biased variance, eps inside the root),
 * channels-last x [n][hw][c] with exactly 4 channels per group (c == 4·groups), 16-byte aligned.
 *   forward: y = act((x − μ_g)·rstd_g·γ_c + β_c); stats [n·groups][2] = (μ, rstd)
 *   backward: dx; dγ / dβ summed over the images in order (part: n·c·2 floats of workspace),
 *             written (accumulate 0) or added onto dgamma / dbeta (accumulate 1) */
int scflow_group_norm_forward(const float* x, const float* gamma, const float* beta, float* y,
                              float* stats, int n, int hw, int c, int groups, float eps, int relu,
                              void* stream);
int scflow_group_norm_backward(const float* dy, const float* x, const float* gamma,
                               const float* beta, const float* stats, float* dx, float* part,
                               float* dgamma, float* dbeta, int n, int hw, int c, int groups,
                               int relu, int accumulate, void* stream);
/* SepConvGRU gate algebra of the training step (raft_decoder.py:235-253), channels-last,
 * c % 4 == 0, zr = the z | r conv's sigmoid output [npix][2c]:
 *   scflow_gru_gate_forward mode 0: out = r·h;  mode 1: out = h + z·(q − h)
 *   scflow_gru_gate_backward_q: dq = dh2·z·(1 − q²); dzr[:, :c] = dh2·(q − h)·z(1 − z);
 *                               dha = dh2·(1 − z)   (dh2 pixel stride sdh2 ≥ c)
 *   scflow_gru_gate_backward_r: dzr[:, c:] = drh·h·r(1 − r); dh = dha + drh·r (drh / dh pixel
 *                               strides sdrh / sdh ≥ c; dh may alias drh: each element is read
 *                               before it is written, by the same thread) */
int scflow_gru_gate_forward(const float* zr, const float* h, const float* q, float* out,
                            long long npix, int c, int mode, void* stream);
int scflow_gru_gate_backward_q(const float* dh2, int sdh2, const float* zr, const float* h,
                               const float* q, float* dq, float* dzr, float* dha, long long npix,
                               int c, void* stream);
int scflow_gru_gate_backward_r(const float* drh, int sdrh, const float* zr, const float* h,
                               const float* dha, float* dzr, float* dh, int sdh, long long npix,
                               int c, void* stream);
/* scflow_col2im: the adjoint of scflow_im2col (same geometry; dx has pixel stride sdx ≥ cin):
 *   dx[n][iy][ix][c] = Σ_{ty,tx: (iy+ph−ty)/s, (ix+pw−tx)/s integral, inside} cols[(n,oy,ox)][(ty·kw+tx)·cin+c]
 * — a fixed-order gather, written (not accumulated).  With cols = dY·Wmat (Wmat[co][(ty·kw+tx)·cin+ci]
 * = w[co][ci][ty][tx]) it is a strided conv's input gradient without zero insertion (training:
 * the stride-2 convs of the encoders and the pose head, resnet.py / pose_head.py:201-211). */
int scflow_col2im(const float* cols, float* dx, int sdx, int n, int h, int w, int cin, int kh, int kw,
                  int stride, int ph, int pw, void* stream);

/* scflow_conv_wgrad: weight (and bias) gradient of a channels-last conv without an im2col
 * matrix — dw[co][ci][ty][tx] (+)= Σ_p dy[p][co] · x[n][oy·s − ph + ty][ox·s − pw + tx][ci],
 * db[co] (+)= Σ_p dy[p][co] (db may be NULL); x = the channel concat of src0 (cin0) and src1
 * (cin1, optional).  Replaces the weight-gradient half of the reference's autograd for every
 * nn.Conv2d on the training path (torch.nn.grad.conv2d_weight, called by
 * SCFlowRefiner.loss → backward, scflow_refiner.py:182-256).  Shapes: 1×1 and 3×3 (stride 1
 * or 2), 1×5 and 5×1 (stride 1); others return SCFLOW_EUNSUPPORTED.  `workspace` holds the
 * per-split partial sums: at least scflow_conv_wgrad_workspace() floats.  The split count
 * follows the device's CU count; the reduction order is fixed (deterministic). */
typedef struct {
  const float* dy;
  int sdy;
  const float* src0;
  int cin0, s0;
  const float* src1;
  int cin1, s1;
  float* dw;
  float* db;
  float* workspace;
  long long workspace_floats;
  int n, h, w, cout, kh, kw, stride, ph, pw;
  int accumulate;
} scflow_wgrad_args;
/* Training: InstanceNorm2d(affine=False) (+ ReLU) of channels-last x [n][hw][c] (c % 4 == 0,
 * c ≤ 256 for the backward), the feature encoder's norms (resnet.py BasicBlock).  Statistics from
 * scflow_enc_stats + scflow_enc_norm_finalize (scale = rstd, shift = −mean·rstd);
 * scflow_in_apply: y = act(x·scale + shift);  scflow_in_backward: dx = rstd·(g − mean(g) −
 * x̂·mean(g·x̂)), g = dy masked by x̂ > 0 when relu — workspace partial: n·chunks·2·c doubles,
 * mm: n·2·c floats. */
int scflow_in_apply(const float* x, const float* scale, const float* shift, float* y, int n, int hw,
                    int c, int relu, void* stream);
/* The residual block's tail in one pass each way (raft_encoder.py BasicBlock: y = relu(norm2(·) +
 * identity)): scflow_in_apply_residual: y = max(x·scale + shift + res, 0);
 * scflow_in_backward_residual: g = dy·(y > 0) → dres = g and dx = the InstanceNorm backward of g
 * (same workspace as scflow_in_backward). */
/* scflow_colsum: out[c] (+)= Σ_r x[r·ld + c] for a row-major [rows][ld] matrix — the bias
 * gradient Σ_p dY[p][c] of the 7×7 convs and the FC layers in training (deterministic: fixed
 * row chunks, then the chunks in order).  workspace: scflow_colsum_workspace(rows, cols) floats
 * (0 for rows ≤ 256: one pass). */
int scflow_colsum(const float* x, int rows, int cols, int ld, float* out, int accumulate,
                  float* workspace, void* stream);
int scflow_colsum_workspace(int rows, int cols);
int scflow_in_apply_residual(const float* x, const float* scale, const float* shift, const float* res,
                             float* y, int n, int hw, int c, void* stream);
int scflow_in_backward_residual(const float* dy, const float* x, const float* scale,
                                const float* shift, const float* y, float* dx, float* dres,
                                double* partial, float* mm, int n, int hw, int c, int chunks,
                                void* stream);
int scflow_in_backward(const float* dy, const float* x, const float* scale, const float* shift,
                       float* dx, double* partial, float* mm, int n, int hw, int c, int chunks,
                       int relu, void* stream);
/* Training: BatchNorm2d in train mode (+ ReLU, + a residual identity added before the ReLU) of
 * channels-last x [m pixels][c] (c % 4 == 0, c ≤ 256), the context encoder's norms (resnet.py
 * BasicBlock, norm_fn 'batch'; torch.nn.functional.batch_norm(training=True)).  The batch
 * statistics in fp64 (the InstanceNorm statistics over one image of m pixels, chunks ≤ m/256
 * pixel chunks), then per channel rstd = 1/√(var + eps), shift = −mean·rstd (x̂ = x·rstd + shift),
 * the folded affine sc = γ·rstd, sh = β − γ·mean·rstd, and — when running_mean / running_var are
 * given — running ← (1 − momentum)·running + momentum·(mean, unbiased var); y = act(x·sc + sh
 * [+ res]) (ReLU when relu or res).  gamma / beta NULL: no affine.  partial: chunks·2·c doubles.
 * scflow_bn_backward: g = dy masked by y > 0 (y given: the residual form, dres = g) or by
 * γ·x̂ + β > 0 (relu), dx = γ·rstd·(g − mean(g) − x̂·mean(g·x̂)), dγ (+)= Σ g·x̂, dβ (+)= Σ g
 * (accumulate); mm: 2·c floats. */
int scflow_bn_forward(const float* x, const float* gamma, const float* beta, const float* res,
                      float* y, float* running_mean, float* running_var, float* rstd, float* shift,
                      float* sc, float* sh, double* partial, long long m, int c, int chunks,
                      float eps, float momentum, int relu, void* stream);
int scflow_bn_backward(const float* dy, const float* x, const float* rstd, const float* shift,
                       const float* gamma, const float* beta, const float* y, float* dx,
                       float* dres, float* dgamma, float* dbeta, double* partial, float* mm,
                       long long m, int c, int chunks, int relu, int accumulate, void* stream);
/* scflow_gemm_f32: batched strided fp32 GEMM on the matrix cores (training-step contractions:
 * the correlation volume's backward, the 7x7 convs' dY^T.cols weight gradient, the pose head's
 * fully connected layers forward/backward; replaces torch.matmul / F.linear there,
 * raft_decoder.py:35-58 and pose_head.py:201-211 adjoints):
 *   C[b][m][n] = alpha * sum_k A[b][m][k] * B[b][k][n] (+ beta * C[b][m][n]) (+ bias)
 * with element strides: A (b, m, k) at b*sab + m*sam + k*sak, B (b, k, n) at b*sbb + k*sbk + n*sbn,
 * C (b, m, n) at b*scb + m*scm + n*scn.  bias_mode 0: none, 1: bias[n], 2: bias[m].  Any strides
 * work; float4 loads are used along a unit-stride dimension when the base and outer strides are
 * 16-byte aligned.  splits > 1 splits K over the grid: workspace holds splits*batch*M*N floats
 * and a second launch sums the splits in order (deterministic); scflow_gemm_f32_splits() gives
 * the split count this build picks for a shape (1 = no workspace needed). */
int scflow_gemm_f32_splits(int batch, int M, int N, int K);
int scflow_gemm_f32(const float* A, const float* B, float* C, const float* bias, int batch, int M,
                    int N, int K, long long sab, long long sam, long long sak, long long sbb,
                    long long sbk, long long sbn, long long scb, long long scm, long long scn,
                    float alpha, float beta, int bias_mode, int splits, float* workspace,
                    void* stream);
int scflow_conv_wgrad_workspace(const scflow_wgrad_args* args, long long* floats);
int scflow_conv_wgrad(const scflow_wgrad_args* args, void* stream);
/* scflow_conv_wgrad_batched: the weight (and bias) gradient summed over `segs` (1..8) equally
 * shaped segments in one launch and one split reduction — the decoder's per-iteration uses of
 * one conv (its 8 refinement iterations under SCFlowRefiner.loss → backward,
 * scflow_refiner.py:182-256).  `args` describes one segment (n images; its dy / src0 / src1 are
 * ignored), dys[i] / src0s[i] / src1s[i] are segment i's bases with args' strides.  Shapes:
 * scflow_conv_wgrad's (Winograd 3×3 / 1×5 / 5×1, 1×1 stride 1–2, the implicit-GEMM 3×3, the
 * thin kernels for ≤ 4 channels on one side); others return SCFLOW_EUNSUPPORTED.  `workspace`: scflow_conv_wgrad_workspace() of args with n·segs
 * images (it sizes the partial sums for any segment count). */
int scflow_conv_wgrad_batched(const scflow_wgrad_args* args, int segs, const float* const* dys,
                              const float* const* src0s, const float* const* src1s, void* stream);
/* scflow_conv_wgrad_plan: host-only — what the weight-gradient launch plan (plan_wgrad,
 * train.hip) decides for `walk`, the argument struct with n = ALL segments' images (what
 * scflow_conv_wgrad_workspace takes), cut into `segs` equal segments; nothing is launched or
 * dereferenced.  segs 1..8: a launch — *kind = the kernel family (SCFLOW_WGRAD_*; NONE when the
 * arguments are invalid or no family takes the shape), *floats = the workspace that launch needs,
 * returns the status scflow_conv_wgrad / _batched answer before launching (SCFLOW_EINVAL for a
 * walk->workspace_floats below *floats, with kind and floats still reported).  segs 0: the
 * workspace query — pointers may be NULL, *floats = the bound that holds for any segment count. */
int scflow_conv_wgrad_plan(const scflow_wgrad_args* walk, int segs, int* kind, long long* floats);
#define SCFLOW_WGRAD_NONE 0
#define SCFLOW_WGRAD_THIN 1   /* wgrad_thin_kernel: ≤ 4 channels on one side, kernels up to 5×5 */
#define SCFLOW_WGRAD_WINO 2   /* wgrad_wino_kernel: Winograd F(2×2,3×3), 3×3 stride 1 pad 1     */
#define SCFLOW_WGRAD_WINO5 3  /* wgrad_wino5_kernel: Winograd F(4,5), 1×5 / 5×1                 */
#define SCFLOW_WGRAD_1X1 4    /* wgrad_1x1_kernel: 1×1 stride 1–2, 128 × 128 tiles              */
#define SCFLOW_WGRAD_GEMM 5   /* wgrad_kernel: the direct implicit GEMM                         */
int scflow_corr_lookup_backward(const float* dout, int out_layout, int out_stride, const float* flow,
                                int flow_layout, float* dpyr, int n, int h, int w, int num_levels,
                                int radius, void* stream);
/* The adjoint of scflow_corr_lookup_masked with respect to the pyramid: scatters
 * mask[m] · dout[m][k] (mask [n·h·w]; the same bits as scflow_corr_lookup_backward fed
 * dout · mask).  No gradient for the mask or the flow.  mask NULL: scflow_corr_lookup_backward. */
int scflow_corr_lookup_backward_masked(const float* dout, int out_layout, int out_stride,
                                       const float* flow, int flow_layout, const float* mask,
                                       float* dpyr, int n, int h, int w, int num_levels, int radius,
                                       void* stream);

/* §8(f)-3 mesh renderer (replaces pytorch3d's MeshRasterizer + HardPhongShader behind
 * models/utils/rendering.py:196-248, configured as scflow_ycbv_real.py:261-274).
 * A batch of n_img images of size×size; image i shows one mesh whose vertices / faces are the
 * i-th block of the packed arrays (pytorch3d's join_meshes_as_batch packing: faces hold packed
 * vertex indices; vert_img / face_img give each packed vertex / face its image).  Outputs
 * (each optional except that images needs normals, colors and the light/material colours):
 *   images [n][size][size][4] RGBA (background colour, alpha 0 where empty),
 *   zbuf [n][size][size] (view depth, −1 empty), pix_to_face (packed face, −1 empty),
 *   bary [n][size][size][3] (perspective-corrected barycentrics, −1 empty).
 * Light placement (Renderer.forward :209-230): SCFLOW_LIGHT_FIXED = light_location (object
 * frame; pytorch3d's default (0, 1, 0)); SCFLOW_LIGHT_PER_IMAGE = R_i·(0, 0, max(z_i − 400, 0)),
 * z_i the image's nearest vertex depth (seperate_lights); SCFLOW_LIGHT_BATCH_ZNEAR =
 * R_i·(0, 0, znear/4), znear = ⌊min depth over the batch / 100⌋·100.  Vertex depths must be
 * positive (objects in front of the camera).  workspace: ≥ scflow_render_workspace() bytes. */
#define SCFLOW_LIGHT_FIXED 0
#define SCFLOW_LIGHT_PER_IMAGE 1
#define SCFLOW_LIGHT_BATCH_ZNEAR 2
typedef struct {
  const float* verts;    /* [total_verts][3] object frame */
  const float* normals;  /* [total_verts][3] (pytorch3d verts_normals) */
  const float* colors;   /* [total_verts][3] vertex colours in [0, 1] */
  const int* faces;      /* [total_faces][3] packed vertex indices */
  const int* vert_img;   /* [total_verts] image of each packed vertex */
  const int* face_img;   /* [total_faces] image of each packed face, non-decreasing (faces packed
                            image by image: the rasteriser bins each image's contiguous range) */
  const float* R;        /* [n_img][3][3] OpenCV rotation (object → camera) */
  const float* t;        /* [n_img][3] */
  const float* K;        /* [n_img][3][3] intrinsics */
  int n_img, size, total_verts, total_faces;
  int light_mode;
  const float* light_location;                  /* [3], SCFLOW_LIGHT_FIXED only */
  const float* ambient;                         /* [3] light·material ambient */
  const float* diffuse;                         /* [3] */
  const float* specular;                        /* [3] */
  float shininess;
  const float* background;                      /* [3] */
  float* images;
  float* zbuf;
  int* pix_to_face;
  float* bary;
  void* workspace;
  long long workspace_bytes;
  float* light_out;      /* optional [n_img][3]: the light location each image was shaded with
                            (object frame) — the reference's PointLights location, :209-230 */
} scflow_render_args;
long long scflow_render_workspace(int n_img, int size, int total_verts);
int scflow_render(const scflow_render_args* args, void* stream);

/* UV-textured meshes on the same renderer (pytorch3d's TexturesUV behind HardPhongShader, what
 * load_objs_as_meshes / join_meshes_as_batch(include_textures=True) give the reference's Renderer
 * for its mesh_ext='obj' configs, rendering.py:64-68, 189-190).  scflow_render_textured is
 * scflow_render with one change: on an image that has a texture map, the texel that enters
 *   rgb = (ambient + diffuse·dif)·texel + specular·spec
 * is not the interpolated vertex colour but the map's bilinear sample at
 *   uv = b0·verts_uvs[faces_uvs[f][0]] + b1·verts_uvs[faces_uvs[f][1]] + b2·verts_uvs[faces_uvs[f][2]]
 * (f the winning face, b its perspective-corrected barycentrics), sampled as TexturesUV.
 * sample_textures does with its defaults (rows flipped, grid_sample bilinear, align_corners=True,
 * padding_mode='border'); on the map as stored, [H][W] with row 0 the image file's first row:
 *   x = clamp(u·(W−1), 0, W−1), y = clamp((1−v)·(H−1), 0, H−1), taps (x0, y0), (x0+1, y0),
 *   (x0, y0+1), (x0+1, y0+1) with the upper indices clamped to the map; a 1×1 map is its texel.
 * Maps are RGBA8 (one dword load per tap; 4 MB for a 1024² map against 16 MB as fp32), texel =
 * byte/255 in fp32, A unread.  Every image samples its own map at that map's own H, W: maps of
 * different sizes in one batch are not padded to a common size (pytorch3d pads; the reference's
 * data has one size).  Alpha, background, zbuf, pix_to_face, bary and light_out are
 * scflow_render's bits, and so is the whole image where tex_offset < 0: in a batch that mixes
 * both kinds scflow_render's own shading launch runs first, over the whole batch, and a second
 * launch then writes the images that have a map.  No mip chain.
 * tex NULL, or every tex_offset < 0: scflow_render, bit for bit.  texels, verts_uvs, faces_uvs:
 * device memory; tex_offset, tex_hw: HOST arrays, read before the launch (they travel to the
 * kernel as launch arguments, 64 images per shading launch; a captured graph therefore bakes the
 * per-image table in: a replay shades with the offsets and sizes given at capture, whatever the
 * host arrays hold by then — capture again when labels or maps change).
 * SCFLOW_EINVAL before any launch: tex_offset NULL; with some tex_offset ≥ 0, a NULL texels / tex_hw / verts_uvs / faces_uvs or
 * total_uvs ≤ 0; a textured image with H or W < 1, an offset that is no multiple of 4 or a map
 * that ends past texel_bytes.  faces_uvs must index [0, total_uvs): device data, not checked. */
typedef struct {
  const unsigned char* texels;  /* device: RGBA8 maps back to back, each [H][W][4], 4-byte aligned */
  long long texel_bytes;        /* size of texels */
  const long long* tex_offset;  /* host [n_img]: byte offset of image i's map; < 0: image i is
                                   untextured (vertex colours) */
  const int* tex_hw;            /* host [n_img][2]: H, W of image i's map */
  const float* verts_uvs;       /* device [total_uvs][2] */
  const int* faces_uvs;         /* device [total_faces][3], parallel to faces: packed uv indices;
                                   unread for untextured images */
  int total_uvs;
} scflow_render_tex;
int scflow_render_textured(const scflow_render_args* args, const scflow_render_tex* tex, void* stream);

/* BOP pose errors (bop_toolkit pose_error.py with the BOP19 settings; the toolkit is what the
 * reference hands its format_results dumps to).  Both calls enqueue on the stream, synchronise
 * nothing, and give bitwise reproducible results (max, min and integer sums only).
 *
 * scflow_pose_err_sym: for estimate i of class l = labels[i], vertices V = points[l][0 ..
 *   counts[l]) (points [num_classes][max_points][3]; the padding past counts[l] is never read) and
 *   symmetry transforms Sym = sym[sym_offset[l] .. sym_offset[l+1]) (sym [total_syms][12], each a
 *   row-major 3×4 [S_R | S_t]; sym_offset [num_classes + 1]; the set holds the identity):
 *     mssd[i] = min_{S ∈ Sym} max_{x ∈ V} ‖(R̂x + t̂) − (R̄(S_R·x + S_t) + t̄)‖₂   (model units)
 *     mspd[i] = the same with both points projected, proj(X) = (K·X)[:2] / (K·X)[2]  (pixels;
 *               no ε guard: depths are positive)
 *   with (R̂, t̂) = R_est / t_est [n][3][3] / [n][3], (R̄, t̄) = R_gt / t_gt, K [n][3][3].  mssd or
 *   mspd may be NULL (not both); mspd needs K.  The call first sets the outputs to +inf on the
 *   stream; +inf stays where counts[l] ≤ 0, the class has no symmetry entry, or l is outside
 *   [0, num_classes).  fp32; no [n][S][P] intermediate.  SCFLOW_EINVAL before any launch, outputs
 *   untouched: a NULL required pointer, both outputs NULL, mspd without K, num_classes /
 *   max_points / total_syms < 1, n < 0.  n = 0: success, nothing enqueued.
 *
 * scflow_vsd_counts: the pixel counts of the visible surface discrepancy of n pairs.  depth_est,
 *   depth_gt [n][h][w]: depth renders of the class's mesh at the two poses (≤ 0: empty);
 *   depth_test [n_frames][h][w]: the sensor depth (0: no measurement), pair i reads frame
 *   frame_index[i]; K [n][3][3] (fx, fy, cx, cy read; no skew); diameter [n], or NULL for costs
 *   that are not normalised; taus [n_taus], 1 ≤ n_taus ≤ 16; delta in depth units.  Per pixel
 *   (x, y) depth D becomes the distance D·sqrt(((x − cx)/fx)² + ((y − cy)/fy)² + 1); with T the
 *   test distance,
 *     vis(M) = ((M − T ≤ delta) or (T == 0)) and (M > 0)                       ('bop19' visibility)
 *     V_gt = vis(dist_gt), V_est = vis(dist_est) or (V_gt and dist_est > 0), I = V_gt ∧ V_est,
 *     U = V_gt ∨ V_est, cost_k = #{p ∈ I : |dist_gt − dist_est| / diameter ≥ taus[k]}
 *   counts [n][2 + n_taus] int = (|U|, |I|, cost_0 …), cleared by the call on the stream; the
 *   caller forms e_k = (cost_k + |U| − |I|) / |U| (1 where |U| = 0).  A frame_index outside
 *   [0, n_frames) leaves that pair's counts 0.  SCFLOW_EINVAL before any launch, counts untouched:
 *   a NULL pointer other than diameter, n < 0, n_frames / h / w < 1, n_taus outside [1, 16];
 *   SCFLOW_EUNSUPPORTED: h·w > 2^30 or n > 65535.  n = 0: success, nothing enqueued. */
int scflow_pose_err_sym(const float* points, const int* counts, int num_classes, int max_points,
                        const float* sym, const int* sym_offset, int total_syms, const int* labels,
                        const float* R_est, const float* t_est, const float* R_gt,
                        const float* t_gt, const float* K, float* mssd, float* mspd, int n,
                        void* stream);
int scflow_vsd_counts(const float* depth_est, const float* depth_gt, const float* depth_test,
                      const int* frame_index, const float* K, const float* diameter,
                      const float* taus, int n_taus, float delta, int* counts, int n, int n_frames,
                      int h, int w, void* stream);

/* Scene visibility: what bop_toolkit's calc_gt_masks / calc_gt_info produce on the CPU with one
 * render per instance (instance masks, visib_fract, the two boxes), for all instances of all
 * frames of a batch in one call.  The definitions are the project's own; parity with the toolkit
 * is unpinned (it is absent): its half-pixel convention, its w = x_max − x_min boxes and its 3×
 * canvas are not reproduced.
 *
 * The mesh table (built once; scflow_amd/scene.py mesh_table): verts [total_verts][3], faces
 * [total_faces][3] with vertex indices local to the class's block, vert_offset / face_offset
 * [num_classes + 1] (class l owns verts [vert_offset[l], vert_offset[l+1]) and the faces likewise;
 * a class without a mesh has an empty range), bounds [num_classes][6] = (min x, y, z, max x, y, z)
 * of the class's vertices.  A face with an index outside its class's block is dropped, unread.
 *
 * Instances: labels [n], frame_index [n] non-decreasing (instances packed frame by frame), R
 * [n][3][3], t [n][3]; K [n_frames][3][3] (fx, fy, cx, cy read; no skew term).
 *
 *   View point X = R·v + t; projected vertex (u, v) = (fx·X/Z + cx, fy·Y/Z + cy).  Pixel (x, y)
 *   samples (x + pixel_offset, y + pixel_offset): with 0, integer coordinates are pixel centres
 *   (metrics.project, the patch code, cv2).
 *   Dropped faces (there is no clipping): a face with any vertex at Z ≤ 0; a face with zero
 *   screen area.
 *   Coverage: a face covers a sample where its three screen-space edge-function weights are > 0.
 *   Depth at a sample: 1 / (w0/Z0 + w1/Z1 + w2/Z2), the weights summing to 1; the nearest face wins.
 *   Canvas: [−margin_x, width + margin_x) × [−margin_y, height + margin_y).  px_count_all and
 *   bbox_obj are taken over the canvas, everything else over the frame.
 *   Distance: M = depth · sqrt(((x − cx)/fx)² + ((y − cy)/fy)² + 1), scflow_vsd_counts' factor.
 *   Test distance T: with depth_test [n_frames][height][width] (mm, 0 = no measurement) the
 *   sensor depth's distance; without it the minimum of M over the frame's instances (mutual
 *   occlusion only), 0 where there is none.
 *   Visibility: an instance is visible at a frame pixel ⇔ M > 0 ∧ (T = 0 ∨ M − T ≤ delta), VSD's
 *   vis above.
 *
 * Outputs, each optional, at least one given:
 *   stats [n][12] int: px_count_all (silhouette pixels on the canvas), px_count_valid (silhouette
 *     pixels in the frame with T > 0; without depth_test the in-frame silhouette), px_count_visib,
 *     bbox_obj (x, y, w, h) over the canvas (x, y may be negative), bbox_visib (x, y, w, h), 0.
 *     Boxes are (x_min, y_min, x_max − x_min + 1, y_max − y_min + 1), (−1, −1, −1, −1) when empty.
 *   inst_id [n_frames][height][width] int: among the visible instances the one with the smallest
 *     M, ties to the lower index; −1 if none.
 *   depth_scene [n_frames][height][width]: the nearest depth over the frame's instances, 0 if none.
 *   depth_inst [n][height][width]: the instance's own depth, 0 where empty.
 *   mask_visib [n][height][width] bytes: 1 where the instance is visible.
 * An instance whose label is outside [0, num_classes), whose class is empty or whose frame_index is
 * outside [0, n_frames) is skipped: counts 0, both boxes (−1, −1, −1, −1), its planes 0.
 * All counters are integers: the results do not depend on any order and are bitwise
 * reproducible, and an output asked for alone has the bits it has in a call with all of them.
 * The call enqueues on the stream and synchronises nothing; it needs no workspace.
 * SCFLOW_EINVAL before any launch, outputs untouched: args NULL, a NULL pointer other than
 * depth_test and the outputs, num_classes / total_verts / total_faces / n_frames / height / width
 * < 1, n < 0, a negative margin, delta < 0 (or NaN), no output given.  SCFLOW_EUNSUPPORTED: a
 * canvas side > 2^24, n_frames > 65535.  n = 0: success, nothing enqueued. */
typedef struct {
  const float* verts; const int* faces;          /* the mesh table */
  const int* vert_offset; const int* face_offset;
  const float* bounds;
  int num_classes, total_verts, total_faces;
  const int* labels; const int* frame_index;     /* [n] */
  const float* R; const float* t;                /* [n][3][3], [n][3] */
  const float* K;                                /* [n_frames][3][3] */
  int n, n_frames, height, width, margin_x, margin_y;
  float pixel_offset, delta;
  const float* depth_test;                       /* optional [n_frames][height][width] */
  int* stats; int* inst_id; float* depth_scene; float* depth_inst; unsigned char* mask_visib;
} scflow_scene_args;
int scflow_scene_visibility(const scflow_scene_args* args, void* stream);

/* Flow validation: the GT flow with its validity filters, and the end-point-error
 * statistics of a predicted flow against it (models/utils/pose.py:92-121, models/utils/flow.py:6-88,
 * raft_refiner_flow_mask.py:239-259).
 *
 * scflow_flow_gt: one launch, one thread per pixel of [n][h][w], any h and w.  The flow source is
 *   one of two: (a) the poses — depth [n][h][w] lifted with (R_ref, t_ref, K) and projected with
 *   (R_gt, t_gt, K), a pixel with depth ≤ 0 getting invalid_num in both channels; the bits are
 *   those of scflow_lift_points + scflow_pose_flow — or (b) flow_in [n][2][h][w] (then K, R_ref,
 *   t_ref, R_gt, t_gt must be NULL).  A filter is selected by its non-NULL pointer; each decides
 *   from the pixel's UNFILTERED flow (fx, fy), so the fused result is that of applying them one
 *   after another.  bad0 = fx ≥ invalid_num ∧ fy ≥ invalid_num.  Sampling coordinates are the
 *   reference's coords_grid, g = (x + fx)·2 / max(w − 1, 1) − 1 (rows likewise), then
 *   torch.grid_sample's with zero padding, in fp32 without contraction:
 *     gt_mask [n][h][w] (mask_dtype 0: bytes / bool, 1: float): bilinear, align_corners=False — on a
 *       grid normalised for align_corners=True, the reference's quirk; invalid where the sample
 *       < 0.9 or bad0.
 *     depth1 [n][h][w] (the GT pose's rendered depth; depth is then depth0): both with
 *       non-positive values read as 0; bilinear, align_corners=True; consistent = |d0 − warped| /
 *       (d0 + 0.1) < depth_thr.  depth_combine SCFLOW_FLOW_DEPTH_OR: invalid where bad0 or not
 *       consistent; SCFLOW_FLOW_DEPTH_REFERENCE: invalid where bad0 AND not consistent, the
 *       reference's expression, which only rewrites pixels that are invalid already.
 *     face_index1 / face_index2 [n][h][w] (face_dtype 0: int32, 1: int64; compared as float32):
 *       nearest (ties to even), align_corners=True; invalid where the sample of face_index2
 *       differs from face_index1 or bad0.
 *   Outputs, each optional, at least one: flow [n][2][h][w], the unfiltered flow; flow_filtered
 *   [n][2][h][w], invalid_num in both channels where a filter says invalid, else the unfiltered
 *   flow's bits.  Out of place: no output may be flow_in or the other output.
 *   SCFLOW_EINVAL before any launch: args NULL, n / h / w < 1, not exactly one flow source, no
 *   output, depth1 without depth, one face map without the other, an unknown dtype or combine, an
 *   aliased output.  SCFLOW_EUNSUPPORTED: h·w ≥ 2^30, n > 65535.
 *
 * scflow_flow_epe: per sample, over the pixels of flow_tgt / flow_pred [n][2][h][w]:
 *   inside = |flow_tgt| < max_flow; valid = inside ∧ (mask NULL ∨ mask ≥ 0.5) (mask [n][h][w]
 *   float); err = |flow_tgt − flow_pred| (fp32: sqrt(dx·dx + dy·dy), no contraction).
 *   counts [n][4] int = the number of valid pixels, then of valid pixels with err < thresh[k];
 *   sums [n][2] double = Σ err over valid pixels, and with occ_pred [n][h][w] Σ over ALL pixels of
 *   |inside − occ_pred| (else 0); err_map [n][h][w] (optional) = err where valid, err·0 elsewhere.
 *   counts and sums come together or not at all (then err_map is required).  The counts are exact;
 *   the sums are fp64 sums of the fp32 terms in a fixed order (per workgroup, then over the
 *   workgroups in a second launch): no floating-point atomics, the same bits in every run.  A
 *   sample without a valid pixel has counts 0 and sums 0.  workspace: 8-byte aligned, at least
 *   scflow_flow_epe_workspace(n, h, w) bytes (a host-side query, no GPU), needed with counts / sums.
 *   SCFLOW_EINVAL / SCFLOW_EUNSUPPORTED as above. */
#define SCFLOW_FLOW_DEPTH_OR 0
#define SCFLOW_FLOW_DEPTH_REFERENCE 1
typedef struct {
  const float* depth;                            /* [n][h][w]: source (a), and depth0 of the depth filter */
  const float* K; const float* R_ref; const float* t_ref; /* source (a) */
  const float* R_gt; const float* t_gt;
  const float* flow_in;                          /* source (b) [n][2][h][w] */
  int n, h, w;
  float invalid_num;
  const void* gt_mask; int mask_dtype;           /* mask filter */
  const float* depth1; float depth_thr; int depth_combine; /* depth filter */
  const void* face_index1; const void* face_index2; int face_dtype; /* face-index filter */
  float* flow; float* flow_filtered;             /* outputs */
} scflow_flow_gt_args;
int scflow_flow_gt(const scflow_flow_gt_args* args, void* stream);

typedef struct {
  const float* flow_tgt; const float* flow_pred; /* [n][2][h][w] */
  const float* mask; const float* occ_pred;      /* optional [n][h][w] */
  int n, h, w;
  float max_flow;
  float thresh[3];
  int* counts; double* sums; float* err_map;     /* outputs */
  void* workspace; long long workspace_bytes;
} scflow_flow_epe_args;
long long scflow_flow_epe_workspace(int n, int h, int w);
int scflow_flow_epe(const scflow_flow_epe_args* args, void* stream);

/* Batched RANSAC-PnP (replaces BaseFlowRefiner.solve_pose's per-sample host loop,
 * models/refiner/base_flow_refiner.py:99-155, over get_2d_3d_corr_by_fw_flow and
 * cv2.solvePnPRansac, models/utils/pose.py:182-249; deliberately not cv2's algorithm — DESIGN.md
 * §12).  Four stages on the caller's stream, no host synchronisation in or between them, every
 * result bitwise reproducible (integer sums are the only unordered ones).  hw = h·w pixels per
 * sample; hyps ≤ SCFLOW_PNP_MAX_HYPS, n·hw < 2^31 and hw ≤ 2^24, else SCFLOW_EUNSUPPORTED.
 *
 * scflow_pnp_workspace: *bytes = the size of scflow_pnp_compact's workspace (host only, no GPU).
 * scflow_pnp_compact: pixel p = y·w + x of sample b is valid when points[b][p].w > 0 (the float4 of
 *   scflow_lift_points: depth > 0) and, with valid != NULL ([n][hw] floats), valid[b][p] != 0.  The
 *   valid pixels' rows (X, Y, Z, x + flow_x, y + flow_y) go to corr[b][0 .. count[b]) in ascending
 *   p (corr [n][hw][5]; later rows are not written), their number to count[b].  flow [n][2][h][w].
 *   workspace: 16-byte aligned, ≥ scflow_pnp_workspace bytes.
 * scflow_pnp_hypotheses: hypothesis h of sample b draws the rows s_k = (lowbias32(((b·hyps + h)·4
 *   + k) ^ seed) · count[b]) >> 32, k = 0..3 (lowbias32: x ^= x>>16; x *= 0x7feb352d; x ^= x>>15;
 *   x *= 0x846ca68b; x ^= x>>16 on 32 bits; samples [n][hyps][4] receives them, may be NULL),
 *   solves Grunert's P3P on rows 0..2 in fp64 and keeps the root whose pose reprojects row 3 best.
 *   Invalid (hyp_valid 0): count[b] < 4, a repeated row, rows 0..2 collinear in the object frame
 *   (sin² of the angle at row 0 ≤ 1e-4), no positive real root, row 3 behind the camera, or a
 *   non-finite value.  hyp [n][hyps][12] = K·[R|t] row-major 3×4, hyp_pose [n][hyps][12] = [R|t];
 *   an invalid hypothesis holds a projection that puts every point behind the camera.  K [n][3][3].
 * scflow_pnp_score: score[b][h] = the number of rows of corr[b] with camera-frame z > 0 and
 *   reprojection error < thr under hyp[b][h] (fp32; tested as |(x, y) − z·(u, v)|² < thr²·z², no
 *   division), 0 where hyp_valid is 0.  score [n][hyps] is cleared by the call.
 * scflow_pnp_refine: per sample the winner (highest score, lowest h), then refine_iters
 *   Gauss-Newton steps on the winner's inliers (the set re-derived from hyp with
 *   scflow_pnp_score's test, fixed) from hyp_pose (its fp32 rotation made orthonormal again in
 *   fp64, Gram-Schmidt on the rows), with the left perturbation R ← exp(ω)·R,
 *   t ← exp(ω)·t + τ: residuals, Jacobians and the 6×6 normal equations in fp64, summed in a
 *   fixed order and solved by Cholesky; a non-positive or non-finite pivot stops and
 *   keeps the last pose.  K must be upper triangular with K[2][2] = 1.  ok[b] = 1 when count[b] ≥
 *   4, the winner is valid, its score ≥ 4 and the result is finite: then R_out / t_out hold the
 *   pose and inliers[b] the winner's score; else R_out / t_out are bit copies of R_ref / t_ref
 *   and inliers[b] = 0.  pose64 (may be NULL) [n][12] doubles receives the same pose before its
 *   rounding to fp32 (R row-major, then t): at t_z ≈ 1 m one fp32 ulp is 6e-5 mm, more than the
 *   refinement's own error. */
#define SCFLOW_PNP_MAX_HYPS 256
int scflow_pnp_workspace(int n, int h, int w, int hyps, long long* bytes);
int scflow_pnp_compact(const float* points, const float* flow, const float* valid, float* corr,
                       int* count, void* workspace, long long workspace_bytes, int n, int h, int w,
                       void* stream);
int scflow_pnp_hypotheses(const float* corr, const int* count, const float* K, float* hyp,
                          float* hyp_pose, int* hyp_valid, int* samples, int n, int hw, int hyps,
                          unsigned seed, void* stream);
int scflow_pnp_score(const float* corr, const int* count, const float* hyp, const int* hyp_valid,
                     int* score, int n, int hw, int hyps, float thr, void* stream);
int scflow_pnp_refine(const float* corr, const int* count, const float* hyp, const float* hyp_pose,
                      const int* hyp_valid, const int* score, const float* K, const float* R_ref,
                      const float* t_ref, float* R_out, float* t_out, int* ok, int* inliers,
                      double* pose64, int n, int hw, int hyps, float thr, int refine_iters,
                      void* stream);

/* Patches from full frames: the reference's test-time formatting ComputeBbox → Crop →
 * Resize → Pad → RemapPose(adapt_intrinsic) → Normalize (datasets/pipelines/geometry_transform.py:
 * 155-500, formatting.py:42-91; keep_ratio=False, aspect_ratio=1, clip_border=False, min_expand=0)
 * as two launches on the caller's stream with no host work between them.
 *
 * scflow_patch_boxes: object i of class labels[i] projects points[labels[i]][0 .. counts[labels[i]])
 *   (points [num_classes][max_points][3]) as K·(R·X + t) in fp32, K = ori_k[i] or, with k_per_frame,
 *   ori_k[frame_index[i]] (frame_index may be NULL without k_per_frame), and reduces the box
 *   bbox[i] = (l, t, r, b).  side = max(r−l, b−t), centre ((l+r)/2, (t+b)/2), half = side·ratio[i]/2;
 *   x1 = trunc(xc − half), x2 = trunc(xc + half), y likewise (toward zero); the crop is inclusive,
 *   cw = x2−x1+1, ch = y2−y1+1, m = max(cw, ch), sf = size/m, nw = (2·cw·size + m) div 2m (nh
 *   likewise), left = (size−nw) div 2, top = (size−nh) div 2.  geom[i] = (x1, y1, x2, y2, nw, nh, left,
 *   top); T[i] = translate(left, top)·diag(sf, sf, 1)·translate(−x1, −y1) and k[i] = T[i]·K as fp32
 *   3×3 products, left to right, each element summed over its three terms in order.  valid[i] = 0
 *   (then geom = 0, T = identity, k = K) when a projected z ≤ 0, the box is not finite or empty,
 *   side·ratio < 1, m > SCFLOW_PATCH_MAX_CROP, the crop does not meet the height × width frame, the
 *   label is outside [0, num_classes) or frame_index[i] outside [0, num_frames) (K = identity then
 *   with k_per_frame).  size: a multiple of 4 in [4, 4096].
 * scflow_patch_extract: out [n][channels][size][size] fp32 from frames [num_frames][height][width]
 *   [channels] (dtype SCFLOW_PATCH_U8 with 1 or 3 channels, SCFLOW_PATCH_F32 with 1) under geom /
 *   valid of the call above.  Crop pixel (i, j) is frame[y1+i][x1+j] inside the frame and pad
 *   outside; output pixel (left+dx, top+dy), dx < nw, dy < nh, is cv2's INTER_LINEAR of the crop:
 *   source x = ((2·dx+1)·cw − nw)/(2·nw) exactly, x0 its floor, fx = remainder/(2·nw) the only rounded
 *   quantity, x0 < 0 → (0, 0), x0 ≥ cw−1 → (cw−1, 0), y likewise, value (1−fy)·((1−fx)·a + fx·b) +
 *   fy·((1−fx)·c + fx·d) in fp32 without contraction; SCFLOW_PATCH_QUANTIZE rounds it with rintf;
 *   SCFLOW_PATCH_NEAREST takes crop[min(dy·ch div nh, ch−1)][min(dx·cw div nw, cw−1)] instead.  Every
 *   other output pixel, and the whole patch of an invalid object or of a geom that is not one, is
 *   pad.  Then (v − mean[c])/std[c] per output channel c, after SCFLOW_PATCH_TO_RGB reversed the
 *   channel order; mean / std: HOST arrays of `channels` floats read by the call, NULL = 0 / 1.
 *   out: 16-byte aligned.  The taps are read directly; with SCFLOW_PATCH_LDS != 0 the two source
 *   rows of an output row are staged in LDS where the crop row fits the budget
 *   (scflow_patch_staged says whether, under the switch's current value: 1 staged, 0 direct); both
 *   routes give the same bits. */
#define SCFLOW_PATCH_MAX_CROP 8192
#define SCFLOW_PATCH_U8 0
#define SCFLOW_PATCH_F32 1
#define SCFLOW_PATCH_TO_RGB 1
#define SCFLOW_PATCH_QUANTIZE 2
#define SCFLOW_PATCH_NEAREST 4
int scflow_patch_boxes(const float* points, const int* counts, const int* labels, const float* R,
                       const float* t, const float* ori_k, const int* frame_index, const float* ratio,
                       float* bbox, int* geom, float* T, float* k, unsigned char* valid, int n,
                       int num_classes, int max_points, int k_per_frame, int num_frames, int height,
                       int width, int size, void* stream);
int scflow_patch_extract(const void* frames, const int* frame_index, const int* geom,
                         const unsigned char* valid, float* out, int n, int num_frames, int height,
                         int width, int channels, int dtype, int size, float pad, const float* mean,
                         const float* std, int flags, void* stream);
int scflow_patch_staged(int cw, int channels, int dtype, int size);

/* Training patches from full frames: the reference's training formatting PoseJitter
 * → ComputeBbox → Crop(size_range) → RandomHSV → RandomNoise → RandomSmooth → Resize → Pad →
 * RemapPose → Normalize (configs/refine_models/scflow_ycbv_real.py:50-93, datasets/pipelines/
 * jitter.py:51-79, geometry_transform.py:232-254, color_transform.py:78-134) as scflow_train_draw →
 * scflow_patch_boxes → scflow_train_patch_extract on the caller's stream with no host work between.
 *
 * Random numbers: stateless Philox4x32-10 (scflow_philox4x32: the host's evaluation of one call,
 *   counter[4], key[2] → out[4]).  key = (seed low, seed high); counter = (index, object, stream |
 *   (step high 32 bits) << 8, step low 32 bits); object = the object's index in the call +
 *   object_offset; stream = SCFLOW_RNG_*; step < 2^56.  u[0,1) = (w >> 8)·2^-24; u(0,1] =
 *   ((w >> 8) + 0.5)·2^-24 in fp32 (the largest word rounds to 1); normals by Box–Muller with the
 *   precise logf / sqrtf / cosf / sinf: words (w0, w1) → z0 = sqrtf(−2·logf(u(w0)))·cosf(2π·u[w1)),
 *   z1 the same with sinf, (w2, w3) → z2 (cos).
 * scflow_train_draw: per object, for try k = 0 .. max_tries−1 (≤ SCFLOW_TRAIN_MAX_TRIES): angles
 *   (a, b, c) = cfg[ANGLE_MEAN] + cfg[ANGLE_STD]·z of the call (0, object, JITTER + k), degrees;
 *   ΔR = Rx(c)·Ry(b)·Rz(a) (scipy's from_euler('zyx')); R = ΔR·R_gt; rot = acos(clip((tr(R·R_gtᵀ) −
 *   1)/2, −1, 1)) in degrees, rejected when > cfg[ANGLE_LIMIT]; Δt = cfg[T_MEAN..] + cfg[T_STD..]·z
 *   of the call (1, object, JITTER + k), rejected when ‖Δt‖ > cfg[TRANS_LIMIT]; add = mean over
 *   points[label][0 .. counts[label]) of ‖(R_gt·X + t_gt) − (R·X + t_gt + Δt)‖ / diameters[label]
 *   (0 for a label without points or diameter), rejected when > cfg[ADD_LIMIT].  A limit below 0
 *   is off.  The first accepted try gives R_ref, t_ref, errors[i] = (add, rot, ‖Δt‖), ok = 1,
 *   tries = k + 1; without one ok = 0, tries = max_tries, the GT pose and zero errors.  ratio[i]
 *   = cfg[RATIO_LO] + u·(cfg[RATIO_HI] − cfg[RATIO_LO]) from word 0 of (0, object, CROP).
 *   aug[i][8] from the words of (0, object, COLOUR): a, b, c = 1 + (2u − 1)·cfg[H_RATIO..],
 *   sigma = u·cfg[NOISE_RATIO]; and of (1, object, COLOUR): ksize = 2·min(int(u·nk), nk − 1) + 1
 *   with nk = (max_kernel_size + 1) div 2 (max_kernel_size ≤ 5), then stage-mask bits
 *   SCFLOW_AUG_HSV / NOISE / BLUR, each set where u ≤ cfg[P_HSV..]; aug[i] = (a, b, c, sigma,
 *   ksize, mask, 0, 0).  cfg: a HOST array of SCFLOW_TRAIN_CFG_LEN floats read by the call.
 * scflow_train_patch_extract: scflow_patch_extract for uint8 × 3 BGR frames (same geometry, validity
 *   re-check, flags TO_RGB / QUANTIZE, mean / std, output; pad an integer level) with the stages of
 *   aug[i] applied to every crop pixel — pad pixels outside the frame included — before the
 *   bilinear resample reads the crop as uint8: HSV (cv2's 8-bit BGR2HSV in integers, gains a, b, c
 *   in fp32 clipped to 179 / 255 / 255 where the gain is ≥ 1, truncated, cv2's 8-bit HSV2BGR in
 *   fp32), noise (level + (z·sigma)·255 clipped to [0, 255] and truncated; z = the three normals
 *   of (y·cw + x, object, NOISE) for B, G, R), box blur (ksize 3 or 5, BORDER_REFLECT_101 at the
 *   crop's edges, (2·Σ + k²) div (2·k²)).  A stage mask of 0 gives scflow_patch_extract's bits.
 *   The augmented crop window a tile of output pixels reads is staged once in LDS where it fits;
 *   otherwise, and with SCFLOW_PATCH_AUG_DIRECT, every tap computes its own window.  Both routes
 *   give the same bits, and neither depends on size or geom[4..8) for the noise a crop pixel gets.
 * scflow_train_patch_extract_bg: the same with the reference's RandomBackground
 *   (color_transform.py:177-244) between the crop and the stages.  pool [num_slots]
 *   [pool_height][pool_width][3] uint8 BGR; pool_sizes (may be NULL: every slot used in full)
 *   [num_slots][2] = the used (height, width) of a slot, top-left aligned, 1 ≤ h ≤ pool_height, 1 ≤ w
 *   ≤ pool_width; masks [num_frames][height][width] uint8, foreground where != 0.  Object i takes a
 *   background where u[0,1) of word 0 of (0, object, SCFLOW_RNG_BACKGROUND) ≤ p, from slot
 *   min(int(u(word 1)·num_slots), num_slots − 1); choice (may be NULL) [n] replaces the draw: −1
 *   none, 0 .. num_slots−1 that slot, anything else none.  chosen[i] = the slot, −1 for none (also
 *   where the slot's pool_sizes row is not a used size).  Under slot b of used size h_b × w_b,
 *   crop pixel (x, y) keeps the frame's level where it lies inside the frame and masks[frame][y1+y]
 *   [x1+x] != 0; every other crop pixel, pad pixels included, is the level of the slot's used
 *   region resampled to the crop's cw × ch as scflow_patch_extract resamples (source coordinates
 *   of x on w_b → cw and of y on h_b → ch, (1−fx)·a + fx·b per row, then the row blend, rintf).
 *   The stages then run on the composite: noise keys and the blur's fold at the crop's edges are
 *   unchanged.  An invalid object draws (chosen is set) but stays a pad patch.  A background with
 *   stage mask 0 is staged like any other window.  p outside [0, 1] (a NaN too), num_slots ≤ 0,
 *   NULL masks / pool / chosen: SCFLOW_EINVAL; pool_height or pool_width above 2^20:
 *   SCFLOW_EUNSUPPORTED.  Without a background an object's bits are scflow_train_patch_extract's. */
#define SCFLOW_TRAIN_CFG_LEN 20
#define SCFLOW_TRAIN_ANGLE_MEAN 0
#define SCFLOW_TRAIN_ANGLE_STD 1
#define SCFLOW_TRAIN_T_MEAN 2  /* x, y, z */
#define SCFLOW_TRAIN_T_STD 5   /* x, y, z */
#define SCFLOW_TRAIN_ANGLE_LIMIT 8
#define SCFLOW_TRAIN_TRANS_LIMIT 9
#define SCFLOW_TRAIN_ADD_LIMIT 10
#define SCFLOW_TRAIN_RATIO_LO 11
#define SCFLOW_TRAIN_RATIO_HI 12
#define SCFLOW_TRAIN_H_RATIO 13 /* h, s, v */
#define SCFLOW_TRAIN_NOISE_RATIO 16
#define SCFLOW_TRAIN_P_HSV 17 /* hsv, noise, blur */
#define SCFLOW_TRAIN_MAX_TRIES 224
#define SCFLOW_RNG_CROP 0
#define SCFLOW_RNG_COLOUR 1
#define SCFLOW_RNG_NOISE 2
#define SCFLOW_RNG_BACKGROUND 3
#define SCFLOW_RNG_JITTER 16 /* + try */
#define SCFLOW_AUG_HSV 1
#define SCFLOW_AUG_NOISE 2
#define SCFLOW_AUG_BLUR 4
#define SCFLOW_PATCH_AUG_DIRECT 8
void scflow_philox4x32(const unsigned int* counter, const unsigned int* key, unsigned int* out);
int scflow_train_draw(const float* points, const int* counts, const int* labels,
                      const float* diameters, const float* R_gt, const float* t_gt, const float* cfg,
                      float* R_ref, float* t_ref, float* errors, unsigned char* ok, int* tries,
                      float* ratio, float* aug, int n, int num_classes, int max_points,
                      int max_tries, int max_kernel_size, unsigned long long seed,
                      unsigned long long step, unsigned int object_offset, void* stream);
int scflow_train_patch_extract(const void* frames, const int* frame_index, const int* geom,
                             const unsigned char* valid, const float* aug, float* out, int n,
                             int num_frames, int height, int width, int size, int pad,
                             const float* mean, const float* std, int flags,
                             unsigned long long seed, unsigned long long step,
                             unsigned int object_offset, void* stream);
int scflow_train_patch_extract_bg(const void* frames, const int* frame_index, const int* geom,
                                  const unsigned char* valid, const float* aug, float* out,
                                  const unsigned char* masks, const unsigned char* pool,
                                  const int* pool_sizes, const int* choice, int* chosen, int n,
                                  int num_frames, int height, int width, int size, int pad,
                                  const float* mean, const float* std, int flags, int num_slots,
                                  int pool_height, int pool_width, float p,
                                  unsigned long long seed, unsigned long long step,
                                  unsigned int object_offset, void* stream);

/* Profiling helper (bench.py roofline timing; no reference equivalent): a one-thread kernel
 * that stores the GPU's constant-rate wall clock (s_memrealtime) into stamps[idx].  Enqueued on
 * the stream of the kernel being timed, before and after it; as an ordinary kernel it is also a
 * node of a captured hipGraph, so every replay re-stamps.  scflow_wallclock_khz: its rate. */
int scflow_timestamp(unsigned long long* stamps, int idx, void* stream);
long long scflow_wallclock_khz(void);

#ifdef __cplusplus
}
#endif
#endif /* SCFLOW_HIP_H */
