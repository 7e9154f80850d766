"""The hot-path HIP ops as ``torch.library`` custom ops ("called from the build's
SCFlowDecoder through torch.library.custom_op wrappers").

Registered under the ``scflow`` namespace, each with a fake (meta) implementation so FX tracing,
``torch.compile`` and ``torch.library.opcheck`` see through them, and the differentiable
ones with their HIP adjoints (``register_autograd``):

=============================  =====================================================  =========
op                             reference                                              backward
=============================  =====================================================  =========
``scflow::corr_pyramid``       CorrelationPyramid.forward, raft_decoder.py:35-58      yes
``scflow::corr_lookup``        CorrLookup.forward, corr_lookup.py:102-136             pyramid
``scflow::pose_update_flow``   get_pose_from_delta_pose + get_flow_from_delta_pose_   no (the
                               and_points, pose.py:66-88,124-169                      decoder
                                                                                      detaches)
``scflow::convex_upsample``    RAFTDecoder._upsample, raft_decoder.py:381-416, and    yes (flow,
                               RAFTDecoderMask.upsample_mask, raft_decoder_mask.py    logits,
                                                                                      occ)
``scflow::pnp_ransac``         solve_pose_by_pnp (cv2.solvePnPRansac), pose.py:203-   no
                               249, batched; another algorithm
``scflow::patch_boxes``        ComputeBbox + the Crop / Resize / Pad / RemapPose       no
                               geometry, geometry_transform.py:155-500
``scflow::extract_patches``    mmcv imcrop, imrescale, impad, imnormalize of the       no
                               same pipeline, all objects in one launch
``scflow::train_draw``         PoseJitter's rejection loop, Crop's size draw and the    no
                               colour transforms' draws, jitter.py:51-79,
                               color_transform.py:78-134
``scflow::patch_extract_aug``  ``extract_patches`` with RandomHSV / RandomNoise /       no
                               RandomSmooth on the crop, in the same launch
``scflow::patch_extract_aug_   the same with RandomBackground before the stages,       no
bg``                           color_transform.py:177-244
``scflow::flow_gt``            get_flow_from_delta_pose_and_depth + filter_flow_by_   no
                               mask / _by_depth / _by_face_index in one launch,
                               pose.py:92-121, flow.py:6-59
``scflow::flow_epe``           cal_epe's per-sample statistics and eval_epe_and_occ's  no
                               occlusion term, flow.py:64-88
=============================  =====================================================  =========

The backward formulas are ops of their own (``scflow::corr_pyramid_backward``,
``scflow::corr_lookup_backward``, ``scflow::convex_upsample_backward``), so AOT autograd traces
the backward graph as well.

The pyramid travels as ONE flat fp32 buffer (levels back to back, each ``[N·H·W, 1, H_l, W_l]``
row-major — ``ops.pyramid_views`` turns it into the reference's list); the modules
``CorrelationPyramid`` / ``CorrLookup`` (modules.py) call these ops.  Every op runs the HIP
kernel on the inputs' current stream; there is no CPU implementation (the product path fails
loudly off-GPU, ``ScflowError``).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import ops

Tensor = torch.Tensor


def pyramid_numel(n: int, h: int, w: int, num_levels: int) -> int:
    """Elements of the flat pyramid buffer: N·H·W maps per level of (H>>l)·(W>>l)."""
    return n * h * w * sum((h >> l) * (w >> l) for l in range(num_levels))


# ------------------------------------------------------------------------------------ a1
@torch.library.custom_op("scflow::corr_pyramid", mutates_args=(), device_types="cuda")
def corr_pyramid(feat1: Tensor, feat2: Tensor, num_levels: int) -> Tensor:
    """feat1, feat2 [N, C, H, W] fp32 → flat pyramid buffer (level 0 = f1ᵀf2/√C, levels 1.. =
    AvgPool2d(2, 2) over the target dims)."""
    buf, _ = ops.corr_pyramid(feat1.contiguous(), feat2.contiguous(), num_levels)
    return buf


@corr_pyramid.register_fake
def _(feat1, feat2, num_levels):
    n, _, h, w = feat1.shape
    return feat1.new_empty(pyramid_numel(n, h, w, num_levels))


def _corr_pyramid_setup(ctx, inputs, output):
    feat1, feat2, num_levels = inputs
    ctx.save_for_backward(feat1, feat2)
    ctx.num_levels = num_levels


@torch.library.custom_op("scflow::corr_pyramid_backward", mutates_args=(), device_types="cuda")
def corr_pyramid_backward(dbuf: Tensor, feat1: Tensor, feat2: Tensor, num_levels: int
                          ) -> Tuple[Tensor, Tensor]:
    """AvgPool adjoint down the levels, then dF1 = F2·dCᵀ, dF2 = F1·dC on the HIP GEMM (the
    training step's adjoint, train/functions.py _CorrPyramid)."""
    n, c, h, w = feat1.shape
    P = h * w
    levels = ops.pyramid_views(dbuf.contiguous(), n, h, w, num_levels)
    g = levels[-1]
    for lv in reversed(levels[:-1]):
        hl, wl = lv.shape[-2:]
        up = torch.zeros_like(lv)
        up[..., : (hl // 2) * 2, : (wl // 2) * 2] = \
            g.repeat_interleave(2, -2).repeat_interleave(2, -1) * 0.25
        g = lv + up
    dC = g.reshape(n, P, P) / (c ** 0.5)
    f1 = feat1.contiguous().view(n, c, P)
    f2 = feat2.contiguous().view(n, c, P)
    df1 = ops.gemm(f2, dC.transpose(1, 2)).view_as(feat1)
    df2 = ops.gemm(f1, dC).view_as(feat2)
    return df1, df2


@corr_pyramid_backward.register_fake
def _(dbuf, feat1, feat2, num_levels):
    return torch.empty_like(feat1, memory_format=torch.contiguous_format), \
        torch.empty_like(feat2, memory_format=torch.contiguous_format)


def _corr_pyramid_backward(ctx, dbuf):
    feat1, feat2 = ctx.saved_tensors
    df1, df2 = corr_pyramid_backward(dbuf, feat1, feat2, ctx.num_levels)
    return df1, df2, None


corr_pyramid.register_autograd(_corr_pyramid_backward, setup_context=_corr_pyramid_setup)


# ------------------------------------------------------------------------------------ a2
@torch.library.custom_op("scflow::corr_lookup", mutates_args=(), device_types="cuda")
def corr_lookup(pyramid: Tensor, flow: Tensor, num_levels: int, radius: int,
                align_corners: bool) -> Tensor:
    """pyramid (flat buffer of ``corr_pyramid``), flow [B, 2, H, W] → [B, L·(2r+1)², H, W]."""
    B, _, H, W = flow.shape
    return ops.corr_lookup(pyramid.contiguous(), flow.contiguous(), B, H, W, num_levels, radius,
                           align_corners=align_corners)


@corr_lookup.register_fake
def _(pyramid, flow, num_levels, radius, align_corners):
    B, _, H, W = flow.shape
    return flow.new_empty(B, num_levels * (2 * radius + 1) ** 2, H, W)


def _corr_lookup_setup(ctx, inputs, output):
    pyramid, flow, num_levels, radius, align_corners = inputs
    ctx.save_for_backward(flow)
    ctx.cfg = (pyramid.numel(), num_levels, radius, align_corners)


@torch.library.custom_op("scflow::corr_lookup_backward", mutates_args=(), device_types="cuda")
def corr_lookup_backward(dout: Tensor, flow: Tensor, numel: int, num_levels: int, radius: int
                         ) -> Tensor:
    """Gradient w.r.t. the pyramid only (the decoder detaches the flow, scflow_decoder.py:193-194):
    the adjoint scatter with grid_sample's tap weights (scflow_corr_lookup_backward,
    align_corners=True)."""
    B, _, H, W = flow.shape
    dpyr = torch.zeros(numel, device=dout.device, dtype=torch.float32)
    # channels-last gradient and flow: the layouts of the training step's lookup backward
    ops.corr_lookup_backward(dout.permute(0, 2, 3, 1).contiguous().view(B * H * W, -1),
                             flow.permute(0, 2, 3, 1).contiguous(), dpyr, B, H, W, num_levels,
                             radius)
    return dpyr


@corr_lookup_backward.register_fake
def _(dout, flow, numel, num_levels, radius):
    return dout.new_empty(numel)


def _corr_lookup_backward(ctx, dout):
    (flow,) = ctx.saved_tensors
    numel, L, r, ac = ctx.cfg
    if not ac:
        raise NotImplementedError("scflow::corr_lookup backward: align_corners=True only "
                                  "(SCFlow's configuration)")
    if ctx.needs_input_grad[1]:
        # grid_sample would also give the sampling coordinates a gradient (corr_lookup.py:
        # 102-136); every SCFlow caller detaches the flow first (scflow_decoder.py:193-194), and a
        # silent zero gradient would be wrong, so an attached flow is an error
        raise NotImplementedError("scflow::corr_lookup backward: no gradient w.r.t. flow — "
                                  "detach the flow (as SCFlowDecoder does)")
    return corr_lookup_backward(dout, flow, numel, L, r), None, None, None, None


corr_lookup.register_autograd(_corr_lookup_backward, setup_context=_corr_lookup_setup)


# ------------------------------------------------------------------------------------ a2, masked
@torch.library.custom_op("scflow::corr_lookup_masked", mutates_args=(), device_types="cuda")
def corr_lookup_masked(pyramid: Tensor, flow: Tensor, mask: Tensor, num_levels: int, radius: int,
                       align_corners: bool) -> Tensor:
    """``corr_lookup`` times the occlusion mask [B, 1, H, W] (the reference's ``mask_corr``,
    scflow_decoder.py:189-207), multiplied where each sample is stored
    (scflow_corr_lookup_masked): → [B, L·(2r+1)², H, W]."""
    B, _, H, W = flow.shape
    return ops.corr_lookup(pyramid.contiguous(), flow.contiguous(), B, H, W, num_levels, radius,
                           align_corners=align_corners, mask=mask.contiguous().view(B * H * W))


@corr_lookup_masked.register_fake
def _(pyramid, flow, mask, num_levels, radius, align_corners):
    B, _, H, W = flow.shape
    return flow.new_empty(B, num_levels * (2 * radius + 1) ** 2, H, W)


def _corr_lookup_masked_setup(ctx, inputs, output):
    pyramid, flow, mask, num_levels, radius, align_corners = inputs
    ctx.save_for_backward(flow, mask)
    ctx.cfg = (pyramid.numel(), num_levels, radius, align_corners)


@torch.library.custom_op("scflow::corr_lookup_masked_backward", mutates_args=(),
                         device_types="cuda")
def corr_lookup_masked_backward(dout: Tensor, flow: Tensor, mask: Tensor, numel: int,
                                num_levels: int, radius: int) -> Tensor:
    """Gradient w.r.t. the pyramid only: the adjoint scatter of mask · dout
    (scflow_corr_lookup_backward_masked, align_corners=True)."""
    B, _, H, W = flow.shape
    dpyr = torch.zeros(numel, device=dout.device, dtype=torch.float32)
    ops.corr_lookup_backward(dout.permute(0, 2, 3, 1).contiguous().view(B * H * W, -1),
                             flow.permute(0, 2, 3, 1).contiguous(), dpyr, B, H, W, num_levels,
                             radius, mask=mask.contiguous().view(B * H * W))
    return dpyr


@corr_lookup_masked_backward.register_fake
def _(dout, flow, mask, numel, num_levels, radius):
    return dout.new_empty(numel)


def _corr_lookup_masked_backward(ctx, dout):
    flow, mask = ctx.saved_tensors
    numel, L, r, ac = ctx.cfg
    if not ac:
        raise NotImplementedError("scflow::corr_lookup_masked backward: align_corners=True only "
                                  "(SCFlow's configuration)")
    if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
        # the same policy as scflow::corr_lookup's flow gradient: every SCFlow configuration
        # detaches both (detach_flow, detach_mask), and a silent zero gradient would be wrong
        raise NotImplementedError("scflow::corr_lookup_masked backward: no gradient w.r.t. flow "
                                  "or mask — detach them (detach_flow / detach_mask)")
    return corr_lookup_masked_backward(dout, flow, mask, numel, L, r), None, None, None, None, None


corr_lookup_masked.register_autograd(_corr_lookup_masked_backward,
                                     setup_context=_corr_lookup_masked_setup)


# ------------------------------------------------------------------------------------ a8 + a10
@torch.library.custom_op("scflow::pose_update_flow", mutates_args=(), device_types="cuda")
def pose_update_flow(drot: Tensor, dt: Tensor, R: Tensor, t: Tensor, K: Tensor, points: Tensor,
                     invalid_num: float, weight: float, depth_transform: str
                     ) -> Tuple[Tensor, Tensor, Tensor]:
    """Δpose (ortho6d [n, 6] or quaternion [n, 4], Δt [n, 3]) applied to (R, t) → (R', t') and
    the pose-induced flow [n, 2, H, W] of the lifted object points [n, H, W, 4] under K."""
    n, H, W, _ = points.shape
    R_out, t_out = torch.empty_like(R), torch.empty_like(t)
    flow = torch.empty(n, 2, H, W, device=R.device, dtype=torch.float32)
    ops.pose_update_flow(drot.contiguous(), dt.contiguous(), R.contiguous(), t.contiguous(),
                         K.contiguous(), points.contiguous(), R_out, t_out, flow, invalid_num,
                         weight, depth_transform)
    return R_out, t_out, flow


@pose_update_flow.register_fake
def _(drot, dt, R, t, K, points, invalid_num, weight, depth_transform):
    n, H, W, _ = points.shape
    return torch.empty_like(R), torch.empty_like(t), R.new_empty(n, 2, H, W)


# ------------------------------------------------------------------------------------ RAFT tail
@torch.library.custom_op("scflow::convex_upsample", mutates_args=(), device_types="cuda")
def convex_upsample(flow: Tensor, logits: Tensor, occ: Optional[Tensor], logit_scale: float,
                    value_scale: float) -> Tuple[Tensor, Tensor]:
    """RAFT's convex ×8 upsampling (RAFTDecoder._upsample, raft_decoder.py:381-416, and
    RAFTDecoderMask.upsample_mask, raft_decoder_mask.py:141-160) with the reference's NCHW
    operands: flow [N, 2, h, w], raw mask logits [N, 576, h, w] (the decoder's ``.25 *`` is
    ``logit_scale``), occ [N, 1, h, w] or None → (value_scale · upsampled flow [N, 2, 8h, 8w],
    upsampled occ [N, 1, 8h, 8w]; an empty tensor without occ).  One scflow_convex_upsample launch
    behind two layout transposes; its adjoint is ``scflow::convex_upsample_backward``."""
    n, _, h, w = flow.shape
    m = n * h * w
    lg = torch.empty(m, logits.shape[1], device=flow.device, dtype=torch.float32)
    ops.nchw_into(logits.contiguous().float(), ops.Chan.whole(lg))
    lr = torch.empty(m, 2, device=flow.device, dtype=torch.float32)
    ops.nchw_into(flow.contiguous().float(), ops.Chan.whole(lr))
    oc = None if occ is None else occ.contiguous().float().view(m, 1)  # C = 1: already pixel-major
    flow_up = torch.empty(n, 2, 8 * h, 8 * w, device=flow.device, dtype=torch.float32)
    occ_up = flow_up.new_empty(0) if occ is None else flow_up.new_empty(n, 1, 8 * h, 8 * w)
    ops.convex_upsample(ops.Chan.whole(lg), lr, None, oc, n, h, w, flow_up,
                        None if occ is None else occ_up, logit_scale=logit_scale,
                        value_scale=value_scale)
    return flow_up, occ_up


@convex_upsample.register_fake
def _(flow, logits, occ, logit_scale, value_scale):
    n, _, h, w = flow.shape
    return flow.new_empty(n, 2, 8 * h, 8 * w), \
        (flow.new_empty(0) if occ is None else flow.new_empty(n, 1, 8 * h, 8 * w))


def _convex_upsample_setup(ctx, inputs, output):
    flow, logits, occ, logit_scale, value_scale = inputs
    ctx.save_for_backward(flow, logits, *(() if occ is None else (occ,)))
    ctx.scales = (logit_scale, value_scale)


@torch.library.custom_op("scflow::convex_upsample_backward", mutates_args=(), device_types="cuda")
def convex_upsample_backward(g_flow: Tensor, g_occ: Optional[Tensor], flow: Tensor, logits: Tensor,
                             occ: Optional[Tensor], logit_scale: float, value_scale: float
                             ) -> Tuple[Tensor, Tensor, Tensor]:
    """The adjoint of ``scflow::convex_upsample`` with its NCHW operands: gradients of the ×8 flow
    [N, 2, 8h, 8w] and the ×8 occlusion [N, 1, 8h, 8w] (None: zero) → (dflow [N, 2, h, w],
    dlogits [N, 576, h, w], docc [N, 1, h, w]; an empty tensor without occ).  One
    scflow_convex_upsample_bwd call (the softmax recomputed from the logits, no float atomics:
    bitwise reproducible) between layout transposes — the training step's adjoint,
    train/functions.py _ConvexUpsample."""
    n, _, h, w = flow.shape
    m = n * h * w
    dev = flow.device
    lg = torch.empty(m, logits.shape[1], device=dev, dtype=torch.float32)
    ops.nchw_into(logits.contiguous().float(), ops.Chan.whole(lg))
    x = torch.empty(m, 2, device=dev, dtype=torch.float32)
    ops.nchw_into(flow.contiguous().float(), ops.Chan.whole(x))
    oc = None if occ is None else occ.contiguous().float().view(m, 1)
    dlg, dx, docc = ops.convex_upsample_backward(
        ops.Chan.whole(lg), x, oc, g_flow.contiguous().float(),
        None if g_occ is None or oc is None else g_occ.contiguous().float(), n, h, w,
        logit_scale=logit_scale, value_scale=value_scale)
    return (ops.chan_to_nchw(ops.Chan.whole(dx), n, h, w),
            ops.chan_to_nchw(ops.Chan.whole(dlg), n, h, w),
            dx.new_empty(0) if docc is None else docc.view(n, 1, h, w))


@convex_upsample_backward.register_fake
def _(g_flow, g_occ, flow, logits, occ, logit_scale, value_scale):
    n, _, h, w = flow.shape
    return flow.new_empty(n, 2, h, w), flow.new_empty(n, logits.shape[1], h, w), \
        (flow.new_empty(0) if occ is None else flow.new_empty(n, 1, h, w))


def _convex_upsample_backward(ctx, g_flow, g_occ):
    flow, logits, *rest = ctx.saved_tensors
    occ = rest[0] if rest else None
    logit_scale, value_scale = ctx.scales
    dflow, dlogits, docc = convex_upsample_backward(g_flow, None if occ is None else g_occ, flow,
                                                    logits, occ, logit_scale, value_scale)
    return dflow, dlogits, (None if occ is None else docc), None, None


convex_upsample.register_autograd(_convex_upsample_backward, setup_context=_convex_upsample_setup)


# ------------------------------------------------------------------------------------ RANSAC-PnP
@torch.library.custom_op("scflow::pnp_ransac", mutates_args=(), device_types="cuda")
def pnp_ransac(flow: Tensor, depth: Tensor, R: Tensor, t: Tensor, K: Tensor,
               valid: Optional[Tensor], hyps: int, thr: float, refine_iters: int, seed: int
               ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Batched RANSAC-PnP on the device (``ops.pnp_ransac``; replaces solve_pose_by_pnp,
    pose.py:203-249, per sample behind ``.cpu().numpy()``): flow [B, 2, H, W], rendered depth
    [B, H, W], reference pose R [B, 3, 3] / t [B, 3], K [B, 3, 3], valid [B, H, W] or None →
    (R [B, 3, 3], t [B, 3], ok [B] bool, inliers [B] int32).  Not differentiable."""
    return ops.pnp_ransac(flow.contiguous().float(), depth.contiguous().float(),
                          R.contiguous().float(), t.contiguous().float(), K.contiguous().float(),
                          valid, hyps, thr, refine_iters, seed)


@pnp_ransac.register_fake
def _(flow, depth, R, t, K, valid, hyps, thr, refine_iters, seed):
    B = flow.shape[0]
    return (R.new_empty(B, 3, 3), t.new_empty(B, 3), R.new_empty(B, dtype=torch.bool),
            R.new_empty(B, dtype=torch.int32))


# ------------------------------------------------------------------------------------ patches
@torch.library.custom_op("scflow::patch_boxes", mutates_args=(), device_types="cuda")
def patch_boxes(points: Tensor, counts: Tensor, labels: Tensor, R: Tensor, t: Tensor, ori_k: Tensor,
                ratio: Tensor, frame_index: Optional[Tensor], k_per_frame: bool, num_frames: int,
                height: int, width: int, size: int
                ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Crop geometry from the projected model points (``ops.patch_boxes``; replaces ComputeBbox,
    Crop / Resize / Pad's bookkeeping and RemapPose's ``adapt_intrinsic``, geometry_transform.py:
    155-500, per object on the host): → (bbox [N, 4], geom [N, 8] int32, T [N, 3, 3], k [N, 3, 3],
    valid [N] uint8).  Integer arguments of any integer dtype.  Not differentiable."""
    i32 = torch.int32
    return ops.patch_boxes(points.contiguous().float(), counts.contiguous().to(i32),
                           labels.contiguous().to(i32), R.contiguous().float(),
                           t.contiguous().float(), ori_k.contiguous().float(),
                           ratio.contiguous().float(), height, width, size,
                           None if frame_index is None else frame_index.contiguous().to(i32),
                           num_frames, k_per_frame)


@patch_boxes.register_fake
def _(points, counts, labels, R, t, ori_k, ratio, frame_index, k_per_frame, num_frames, height,
      width, size):
    n = labels.shape[0]
    return (R.new_empty(n, 4, dtype=torch.float32), R.new_empty(n, 8, dtype=torch.int32),
            R.new_empty(n, 3, 3, dtype=torch.float32), R.new_empty(n, 3, 3, dtype=torch.float32),
            R.new_empty(n, dtype=torch.uint8))


@torch.library.custom_op("scflow::extract_patches", mutates_args=(), device_types="cuda")
def extract_patches(frames: Tensor, frame_index: Tensor, geom: Tensor, valid: Tensor, size: int,
                    pad: float, mean: Optional[List[float]], std: Optional[List[float]],
                    to_rgb: bool, quantize: bool, nearest: bool) -> Tensor:
    """Crop → Resize → Pad → Normalize of N patches in one launch (``ops.extract_patches``;
    replaces mmcv's imcrop / imrescale / impad / imnormalize per object on the host): frames
    [F, H, W, C] uint8 or float32 → [N, C, size, size] float32.  Not differentiable."""
    return ops.extract_patches(frames.contiguous(), frame_index.contiguous().to(torch.int32),
                               geom.contiguous(), valid.contiguous(), size, pad, mean, std, to_rgb,
                               quantize, nearest)


@extract_patches.register_fake
def _(frames, frame_index, geom, valid, size, pad, mean, std, to_rgb, quantize, nearest):
    return frames.new_empty(frame_index.shape[0], frames.shape[3], size, size, dtype=torch.float32)


@torch.library.custom_op("scflow::train_draw", mutates_args=(), device_types="cuda")
def train_draw(points: Tensor, counts: Tensor, labels: Tensor, diameters: Tensor, R_gt: Tensor,
               t_gt: Tensor, cfg: List[float], max_kernel_size: int, max_tries: int, seed: int,
               step: int, object_offset: int
               ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Pose jitter, crop ratio and colour parameters from the counter-based generator
    (``ops.train_draw``; replaces PoseJitter's rejection loop, jitter.py:51-79, Crop's size draw,
    geometry_transform.py:232-254, and the draws of RandomHSV / RandomNoise / RandomSmooth,
    color_transform.py:78-134, per object on the host): ``cfg`` in the order of ``_lib.TRAIN_CFG``
    → (R_ref, t_ref, errors [N, 3], ok [N] uint8, tries [N] int32, ratio [N], aug [N, 8]).
    Not differentiable."""
    from ._lib import TRAIN_CFG
    i32 = torch.int32
    d = dict(zip(TRAIN_CFG, cfg), max_kernel_size=max_kernel_size)
    return ops.train_draw(points.contiguous().float(), counts.contiguous().to(i32),
                          labels.contiguous().to(i32), diameters.contiguous().float(),
                          R_gt.contiguous().float(), t_gt.contiguous().float(), d, seed, step,
                          object_offset, max_tries)


@train_draw.register_fake
def _(points, counts, labels, diameters, R_gt, t_gt, cfg, max_kernel_size, max_tries, seed, step,
      object_offset):
    n, f32 = labels.shape[0], torch.float32
    return (R_gt.new_empty(n, 3, 3, dtype=f32), R_gt.new_empty(n, 3, dtype=f32),
            R_gt.new_empty(n, 3, dtype=f32), R_gt.new_empty(n, dtype=torch.uint8),
            R_gt.new_empty(n, dtype=torch.int32), R_gt.new_empty(n, dtype=f32),
            R_gt.new_empty(n, 8, dtype=f32))


@torch.library.custom_op("scflow::patch_extract_aug", mutates_args=(), device_types="cuda")
def patch_extract_aug(frames: Tensor, frame_index: Tensor, geom: Tensor, valid: Tensor, aug: Tensor,
                      size: int, seed: int, step: int, object_offset: int, pad: int,
                      mean: Optional[List[float]], std: Optional[List[float]], to_rgb: bool,
                      quantize: bool) -> Tensor:
    """Crop → RandomHSV → RandomNoise → RandomSmooth → Resize → Pad → Normalize of N patches in one
    launch (``ops.extract_patches_aug``; replaces cv2 / mmcv per object on the host,
    color_transform.py:78-134): frames [F, H, W, 3] uint8 BGR → [N, 3, size, size] float32.  Not
    differentiable."""
    return ops.extract_patches_aug(frames.contiguous(), frame_index.contiguous().to(torch.int32),
                                   geom.contiguous(), valid.contiguous(), aug.contiguous().float(),
                                   size, seed, step, object_offset, pad, mean, std, to_rgb,
                                   quantize)


@patch_extract_aug.register_fake
def _(frames, frame_index, geom, valid, aug, size, seed, step, object_offset, pad, mean, std, to_rgb,
      quantize):
    return frames.new_empty(frame_index.shape[0], 3, size, size, dtype=torch.float32)


@torch.library.custom_op("scflow::patch_extract_aug_bg", mutates_args=(), device_types="cuda")
def patch_extract_aug_bg(frames: Tensor, masks: Tensor, frame_index: Tensor, geom: Tensor,
                         valid: Tensor, aug: Tensor, backgrounds: Tensor,
                         background_sizes: Optional[Tensor], background_index: Optional[Tensor],
                         p: float, size: int, seed: int, step: int, object_offset: int, pad: int,
                         mean: Optional[List[float]], std: Optional[List[float]], to_rgb: bool,
                         quantize: bool) -> Tuple[Tensor, Tensor]:
    """``patch_extract_aug`` with RandomBackground between the crop and the colour stages, in the
    same launch (``ops.extract_patches_aug_bg``; replaces cv2.resize + a masked copy per object on
    the host, color_transform.py:177-244): → (patches [N, 3, size, size] float32, the slot every
    object got [N] int32, −1 for none).  Not differentiable."""
    i32 = torch.int32
    sizes = None if background_sizes is None else background_sizes.contiguous().to(i32)
    index = None if background_index is None else background_index.contiguous().to(i32)
    return ops.extract_patches_aug_bg(frames.contiguous(), masks.contiguous(),
                                      frame_index.contiguous().to(i32), geom.contiguous(),
                                      valid.contiguous(), aug.contiguous().float(),
                                      backgrounds.contiguous(), size, seed, step, object_offset, p,
                                      sizes, index, pad, mean, std, to_rgb, quantize)


@patch_extract_aug_bg.register_fake
def _(frames, masks, frame_index, geom, valid, aug, backgrounds, background_sizes, background_index,
      p, size, seed, step, object_offset, pad, mean, std, to_rgb, quantize):
    n = frame_index.shape[0]
    return (frames.new_empty(n, 3, size, size, dtype=torch.float32),
            frames.new_empty(n, dtype=torch.int32))


# ------------------------------------------------------------------------------------ flow validation
@torch.library.custom_op("scflow::flow_gt", mutates_args=(), device_types="cuda")
def flow_gt(depth: Optional[Tensor], K: Optional[Tensor], R_ref: Optional[Tensor],
            t_ref: Optional[Tensor], R_gt: Optional[Tensor], t_gt: Optional[Tensor],
            flow_in: Optional[Tensor], invalid_num: float, gt_mask: Optional[Tensor],
            depth1: Optional[Tensor], depth_thr: float, depth_combine: str,
            face_index1: Optional[Tensor], face_index2: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """The GT flow and its validity filters in one launch (``ops.flow_gt``; replaces
    get_flow_from_delta_pose_and_depth, pose.py:92-121, and filter_flow_by_mask / _by_depth /
    _by_face_index, flow.py:6-59): the poses with depth [N, H, W], or ``flow_in`` [N, 2, H, W] (then
    ``depth`` is only the depth filter's depth0) → (flow, filtered flow), both [N, 2, H, W].  Not
    differentiable."""
    return ops.flow_gt(depth, K, R_ref, t_ref, R_gt, t_gt, flow_in, invalid_num, gt_mask, depth1,
                       depth_thr, depth_combine, face_index1, face_index2)


@flow_gt.register_fake
def _(depth, K, R_ref, t_ref, R_gt, t_gt, flow_in, invalid_num, gt_mask, depth1, depth_thr,
      depth_combine, face_index1, face_index2):
    if flow_in is not None:
        n, _, h, w = flow_in.shape
        like = flow_in
    else:
        n, h, w = depth.shape
        like = depth
    return (like.new_empty(n, 2, h, w, dtype=torch.float32),
            like.new_empty(n, 2, h, w, dtype=torch.float32))


@torch.library.custom_op("scflow::flow_epe", mutates_args=(), device_types="cuda")
def flow_epe(flow_tgt: Tensor, flow_pred: Tensor, mask: Optional[Tensor], max_flow: float,
             threshs: List[float], occ_pred: Optional[Tensor], want_map: bool, want_stats: bool
             ) -> Tuple[Tensor, Tensor, Tensor]:
    """End-point-error statistics per sample (``ops.flow_epe``; replaces cal_epe, flow.py:64-88, and
    eval_epe_and_occ's occlusion term): → (counts [N, 4] int32, sums [N, 2] float64, error map
    [N, H, W]); what is not wanted is an empty tensor.  Not differentiable."""
    counts, sums, emap = ops.flow_epe(flow_tgt, flow_pred, mask, max_flow, threshs, occ_pred,
                                      want_stats, want_map)
    e = flow_tgt.new_empty(0)
    return (e.int() if counts is None else counts, e.double() if sums is None else sums,
            e if emap is None else emap)


@flow_epe.register_fake
def _(flow_tgt, flow_pred, mask, max_flow, threshs, occ_pred, want_map, want_stats):
    n, _, h, w = flow_tgt.shape
    return (flow_tgt.new_empty((n, 4) if want_stats else (0,), dtype=torch.int32),
            flow_tgt.new_empty((n, 2) if want_stats else (0,), dtype=torch.float64),
            flow_tgt.new_empty((n, h, w) if want_map else (0,), dtype=torch.float32))
