"""Training forward of SCFlowRefiner on the HIP autograd Functions.

``refiner_train_forward`` reproduces ``SCFlowRefiner.loss`` (models/refiner/scflow_refiner.py:
182-256) for synthetic batches: shared feature encoder on real + rendered images, context
encoder (BatchNorm in train mode), the decoder loop with the configured detaches
(detach_flow / detach_pose / detach_depth_for_xy, scflow_decoder.py:193-236) and back-prop
through the 8 GRU steps, then the three sequence losses.  Activations are channels-last; every
convolution is ``conv2d_nhwc`` (HIP forward + backward); the correlation pyramid and lookup are
HIP Functions; the detached per-iteration geometry (2D-3D lift, pose-induced flow, flow
downsampling, GT flow) runs on the inference kernels without autograd.  Normalisations,
activations, the GRU gate algebra, the pose update and the losses are torch ops (pointwise /
per-sample); FCs are plain library GEMMs.

``raft_refiner_train_forward`` does the same for the reference's RAFT + PnP baseline
(``RAFTRefinerFlowMask.loss`` / ``RAFTRefinerFlow.loss``, models/refiner/
raft_refiner_flow_mask.py:167-220) on the same pieces: ``raft_decoder_train`` restates the RAFT
decoders' loop (flow detached every iteration, occlusion head, raw mask logits) and upsamples
through ``convex_upsample`` (scflow_convex_upsample forward, scflow_convex_upsample_bwd backward);
the flow and occlusion sequence losses are the torch restatements of losses.py with the weights
of the refiner's stored loss configs.  The two forwards share ``_encode_images``, ``_gt_flow`` and,
inside the decoder loops, ``_motion_features`` and ``_hidden_heads``.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from .. import ops
from ..ops import Chan
from .functions import (ResidualGrad, batch_norm_nhwc, begin_forward, bn_fusable, conv2d_nhwc,
                        conv2d_nhwc_split, convex_upsample, corr_lookup, corr_pyramid,
                        dual_conv2d_nhwc, group_norm_nhwc, gru_step, instance_norm_nhwc,
                        instance_norm_residual_relu_nhwc, linear, pose_update6, share_weight,
                        upsample_bilinear_ac)
from .losses import (LowRes, filter_flow_by_mask, flow_l1_loss, flow_valid, mask_l1_loss, matmul3,
                     refine_losses, sequence_loss)

Tensor = torch.Tensor
_GRU_FUSED = os.environ.get("SCFLOW_TRAIN_GRU_FUSED", "1") != "0"  # A/B switch (tuning)
_FUSED_LOSS = os.environ.get("SCFLOW_TRAIN_FUSED_LOSS", "1") != "0"  # A/B switch (tuning)
_GN_FUSED = os.environ.get("SCFLOW_TRAIN_GN_FUSED", "1") != "0"  # A/B switch (tuning)
_RES_GRAD = os.environ.get("SCFLOW_TRAIN_RES_GRAD", "1") != "0"  # A/B switch (tuning)
_BN_FUSED = os.environ.get("SCFLOW_TRAIN_BN_FUSED", "1") != "0"  # A/B switch (tuning)
_HEADS_FUSED = os.environ.get("SCFLOW_TRAIN_HEADS_FUSED", "1") != "0"  # A/B switch (tuning)


def _act(x: Tensor, act) -> Tensor:
    if act == "ReLU":
        return torch.relu(x)
    if act == "Sigmoid":
        return torch.sigmoid(x)
    if act == "Tanh":
        return torch.tanh(x)
    return x


def _cm(x: Tensor, m, x1: Tensor = None) -> Tensor:
    """mmcv ConvModule (conv → act, fused; the decoder's ConvModules have no norm); ``x1``: a
    second input concatenated along channels (read in place)."""
    c = m.conv
    return conv2d_nhwc(x, c.weight, c.bias, c.stride[0], c.padding, act=m.act_type, x1=x1)


def _conv(x: Tensor, c, res_grad=None) -> Tensor:
    if res_grad is None:
        return conv2d_nhwc(x, c.weight, c.bias, c.stride[0], c.padding)
    return conv2d_nhwc(x, c.weight, c.bias, c.stride[0], c.padding, res_grad=res_grad)


# ------------------------------------------------------------------------------- encoders
def _norm(x: Tensor, mod, relu: bool = False) -> Tensor:
    """InstanceNorm2d (affine=False; HIP statistics / apply / backward, the ReLU fused) or
    BatchNorm2d (train mode: batch statistics, running-stat update) on a channels-last tensor."""
    if isinstance(mod, torch.nn.InstanceNorm2d):
        c = x.shape[-1]
        if x.is_cuda and c % 4 == 0 and c <= 256 and not mod.affine:
            return instance_norm_nhwc(x, mod.eps, relu)
        m = x.mean(dim=(1, 2), keepdim=True)
        v = x.var(dim=(1, 2), unbiased=False, keepdim=True)
        y = (x - m) / torch.sqrt(v + mod.eps)
        return torch.relu(y) if relu else y
    if _BN_FUSED and bn_fusable(mod, x):
        return batch_norm_nhwc(x, mod, relu)
    y = F.batch_norm(x.permute(0, 3, 1, 2), mod.running_mean, mod.running_var, mod.weight, mod.bias,
                     training=mod.training, momentum=mod.momentum, eps=mod.eps)
    if mod.training and mod.num_batches_tracked is not None:
        mod.num_batches_tracked.add_(1)
    y = y.permute(0, 2, 3, 1)
    return torch.relu(y) if relu else y


def encoder_train(enc, x_nhwc: Tensor) -> Tensor:
    """RAFTEncoder.forward (raft_encoder.py:286-314) with autograd; channels-last in and out."""
    x = _norm(_conv(x_nhwc, enc.conv1), enc.norm1, relu=True)
    for name in enc.res_layers:
        for blk in getattr(enc, name):
            n2 = blk.norm2
            in_tail = (isinstance(n2, torch.nn.InstanceNorm2d) and not n2.affine and x.is_cuda
                       and x.shape[-1] % 4 == 0 and x.shape[-1] <= 256)
            bn_tail = _BN_FUSED and bn_fusable(n2, x)
            fused_tail = in_tail or bn_tail
            # identity block: its input's two gradients (conv1's dX, the identity) summed in
            # conv1's dX epilogue (ResidualGrad)
            rg = ResidualGrad() if (fused_tail and blk.downsample is None and _RES_GRAD and
                                    blk.conv1.stride[0] == 1) else None
            out = _norm(_conv(x, blk.conv1, rg), blk.norm1, relu=True)
            ident = x if blk.downsample is None else _norm(_conv(x, blk.downsample[0]), blk.downsample[1])
            y2 = _conv(out, blk.conv2)
            if fused_tail and y2.shape[-1] % 4 == 0 and y2.shape[-1] <= 256 and ident.shape == y2.shape:
                if in_tail:
                    x = instance_norm_residual_relu_nhwc(y2, ident, n2.eps, rg)  # norm + sum + ReLU
                else:
                    x = batch_norm_nhwc(y2, n2, res=ident, res_grad=rg)
            else:
                x = torch.relu(_norm(y2, n2) + ident)
    return _conv(x, enc.conv2)


# ------------------------------------------------------------------------------- pose head
def pose_head_train(head, x: Tensor, label: Tensor) -> Tuple[Tensor, Tensor]:
    """MultiClassPoseHead.forward (pose_head.py:201-211), label[0] quirk kept."""
    for m in head.conv_layers:
        c = m.conv
        y = conv2d_nhwc(x, c.weight, c.bias, c.stride[0], c.padding)
        gn = m.gn
        if y.is_cuda and _GN_FUSED and gn.affine and y.shape[-1] == 4 * gn.num_groups:
            x = group_norm_nhwc(y, gn.weight, gn.bias, gn.num_groups, gn.eps, relu=True)
            continue
        y = F.group_norm(y.permute(0, 3, 1, 2), gn.num_groups, gn.weight, gn.bias, gn.eps)
        x = torch.relu(y).permute(0, 2, 3, 1)
    v = x.permute(0, 3, 1, 2).reshape(x.shape[0], -1)  # nn.Flatten of NCHW
    for fc in head.fc_layers:
        v = torch.relu(linear(v, fc[0].weight, fc[0].bias))
    n = v.shape[0]
    t = linear(v, head.translation_pred.weight, head.translation_pred.bias).view(n, head.num_class, 3)
    r = linear(v, head.rotation_pred.weight, head.rotation_pred.bias).view(
        n, head.num_class, head.rotation_out_channels)
    # index_select(dim=1, index=label)[:, 0]: every sample takes class label[0] (the quirk), as a
    # gather whose backward is a plain scatter-add (index_select's index_add backward: ~48 µs)
    lab = label[:1].view(1, 1, 1)
    t = t.gather(1, lab.expand(n, 1, 3))[:, 0]
    r = r.gather(1, lab.expand(n, 1, r.shape[-1]))[:, 0]
    return r, t


# ------------------------------------------------------------------------------- pose maths
def _normalize(v: Tensor) -> Tensor:
    return v / v.norm(dim=1, keepdim=True).clamp_min(1e-12)


def pose_update(drot: Tensor, dt: Tensor, R: Tensor, t: Tensor, weight: float = 10.0,
                depth_transform: str = "exp", detach_depth_for_xy: bool = True) -> Tuple[Tensor, Tensor]:
    """get_pose_from_delta_pose + get_rotation_matrix_from_ortho6d (pose.py:124-169); a [n, 4]
    drot is a quaternion (x, y, z, w; pose.py:132-133, see oracle.rotation_from_quaternion_xyzw)."""
    if drot.shape[1] == 6 and drot.is_cuda and depth_transform in ("exp", "linear"):
        return pose_update6(drot, dt, R, t, weight, depth_transform == "exp", detach_depth_for_xy)
    if drot.shape[1] == 4:
        q = drot / drot.norm(dim=1, keepdim=True).clamp_min(1e-12)
        qx, qy, qz, qw = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        tx, ty, tz = 2.0 * qx, 2.0 * qy, 2.0 * qz
        one = torch.ones_like(qx)
        D = torch.stack([one - (ty * qy + tz * qz), ty * qx - tz * qw, tz * qx + ty * qw,
                         ty * qx + tz * qw, one - (tx * qx + tz * qz), tz * qy - tx * qw,
                         tz * qx - ty * qw, tz * qy + tx * qw, one - (tx * qx + ty * qy)],
                        dim=-1).view(-1, 3, 3)
        Rd = matmul3(D, R)
    else:
        x = _normalize(drot[:, 0:3])
        z = _normalize(torch.cross(x, drot[:, 3:6], dim=1))
        y = torch.cross(z, x, dim=1)
        Rd = matmul3(torch.stack([x, y, z], dim=2), R)
    vz = t[:, 2] / torch.exp(dt[:, 2]) if depth_transform == "exp" else t[:, 2] * (dt[:, 2] + 1)
    vzxy = vz.detach() if detach_depth_for_xy else vz
    vx = vzxy * (dt[:, 0] / weight + t[:, 0] / t[:, 2])
    vy = vzxy * (dt[:, 1] / weight + t[:, 1] / t[:, 2])
    return Rd, torch.stack([vx, vy, vz], dim=-1)


# ------------------------------------------------------------------------------- decoder
def check_train_flags(dec) -> None:
    """The decoder flags the training path supports, checked before any device work:
    detach_flow=True, and detach_mask=True whenever mask_flow / mask_corr is set (every shipped
    config, configs/refine_models/*.py) — the lookup and the flow branch give the flow and the
    mask no gradient."""
    if not dec.detach_flow:
        raise NotImplementedError("training path follows the configured decoder: detach_flow=True "
                                  "(scflow_ycbv_real.py:213-218)")
    if (dec.mask_flow or dec.mask_corr) and not dec.detach_mask:
        raise NotImplementedError("training with mask_flow / mask_corr needs detach_mask=True: "
                                  "detach_mask=False would need the gradient with respect to the "
                                  "mask through the lookup and the flow branch, which is not "
                                  "implemented")


def _hoist_context(gru, cxt: Tensor, hc: int, cc: int):
    """The loop-invariant context contribution of every GRU conv, once per forward (its gradient
    is the sum over the iterations, so dgrad/wgrad of the context part also run once).  Returns
    (per-conv (w_zr, w_q, padding) without the context's input channels, per-conv (z|r, q)
    pre-activation maps)."""
    it_w, ctx_pre = [], []
    for zc, rc, qc in zip(gru.conv_z, gru.conv_r, gru.conv_q):
        z, rr, q = zc.conv, rc.conv, qc.conv
        wzr = torch.cat([z.weight, rr.weight], 0)
        bzr = torch.cat([z.bias, rr.bias], 0)
        ctx_pre.append((conv2d_nhwc(cxt, wzr[:, hc:hc + cc], bzr, 1, q.padding),
                        conv2d_nhwc(cxt, q.weight[:, hc:hc + cc], q.bias, 1, q.padding)))
        w_zr = torch.cat([wzr[:, :hc], wzr[:, hc + cc:]], 1)
        w_q = torch.cat([q.weight[:, :hc], q.weight[:, hc + cc:]], 1)
        if _GRU_FUSED:  # one batched weight gradient over the iterations' uses
            w_zr, w_q = share_weight(w_zr), share_weight(w_q)
        it_w.append((w_zr, w_q, q.padding))
    return it_w, ctx_pre


def _gru_iteration(h: Tensor, motion: Tensor, it_w, ctx_pre, hc: int) -> Tensor:
    for (w_zr, w_q, pad), (pre_zr, pre_q) in zip(it_w, ctx_pre):  # SeqConv: 1×5 then 5×1
        if _GRU_FUSED:
            h = gru_step(h, motion, w_zr, w_q, pre_zr, pre_q, pad)  # (1 − z)·h + z·q
        else:  # the same step as separate autograd ops (A/B reference)
            z, rg = conv2d_nhwc_split(h, w_zr, hc, None, 1, pad, act="Sigmoid", x1=motion,
                                      bias_map=pre_zr)
            qq = conv2d_nhwc(rg * h, w_q, None, 1, pad, act="Tanh", x1=motion, bias_map=pre_q)
            h = torch.lerp(h, qq, z)
    return h


def _motion_features(enc, corr: Tensor, flow_in: Tensor) -> Tensor:
    """MotionEncoder.forward (raft_decoder.py:61-166) without its final cat: corr_net and flow_net,
    then out_net on their outputs (the first conv reads both in place)."""
    c = corr
    for m in enc.corr_net:
        c = _cm(c, m)
    f = flow_in
    for m in enc.flow_net:
        f = _cm(f, m)
    out = _cm(c, enc.out_net[0], x1=f)
    for m in enc.out_net[1:]:
        out = _cm(out, m)
    return out


def _hidden_heads(h: Tensor, heads) -> List[Tensor]:
    """The XHeads' hidden ConvModules on the GRU state; the first two as one launch each way where
    ``dual_conv2d_nhwc`` allows (one 3×3 layer each, same shape and activation)."""
    def fusable(a, b):
        la, lb = a.layers, b.layers
        return (_HEADS_FUSED and h.is_cuda and len(la) == 1 and len(lb) == 1
                and la[0].conv.kernel_size == lb[0].conv.kernel_size
                and la[0].conv.padding == lb[0].conv.padding and la[0].conv.stride == (1, 1)
                and lb[0].conv.stride == (1, 1) and la[0].act_type == lb[0].act_type
                and (la[0].conv.bias is None) == (lb[0].conv.bias is None))
    outs, rest = [], list(heads)
    if len(rest) >= 2 and fusable(rest[0], rest[1]):
        a, b = rest[0].layers[0], rest[1].layers[0]
        outs += list(dual_conv2d_nhwc(h, a.conv.weight, a.conv.bias, b.conv.weight, b.conv.bias,
                                      a.conv.padding, a.act_type))
        rest = rest[2:]
    for hd in rest:
        x = h
        for m in hd.layers:
            x = _cm(x, m)
        outs.append(x)
    return outs


def decoder_train(dec, feat_render: Tensor, feat_real: Tensor, h: Tensor, cxt: Tensor, R0: Tensor,
                  t0: Tensor, depth: Tensor, K: Tensor, label: Tensor, iters: int,
                  invalid_flow_num: float = 0.0) -> Tuple[List[Tensor], ...]:
    """SCFlowDecoder.forward with autograd (scflow_decoder.py:151-252); features channels-last
    [N, h, w, C].  Returns (flow_from_pose, flow_from_pred, R, t, mask, Δrot, Δt) lists."""
    check_train_flags(dec)
    masked = dec.mask_flow or dec.mask_corr
    N, hh, ww, _ = feat_render.shape
    _, H, W = depth.shape
    dt = feat_render.dtype
    L, r = dec.num_levels, dec.radius
    scale = 2 ** (L - 1)
    pyr = corr_pyramid(feat_render.permute(0, 3, 1, 2), feat_real.permute(0, 3, 1, 2), L)
    depth = depth.contiguous().to(dt)
    K = K.contiguous().to(dt)
    with torch.no_grad():
        points = ops.lift_points(depth, K, R0.contiguous().to(dt), t0.contiguous().to(dt))
    flow_full = torch.zeros(N, 2, H, W, device=depth.device, dtype=dt)
    R, t = R0.to(dt), t0.to(dt)
    label = label.long()
    outs = ([], [], [], [], [], [], [])
    enc = dec.encoder
    gru = dec.gru
    hc, cc = dec.h_channels, dec.cxt_channels
    it_w, ctx_pre = _hoist_context(gru, cxt, hc, cc)
    mask = None
    for _ in range(iters):
        # occlusion masking (scflow_decoder.py:189-207): the previous iteration's low-resolution
        # mask, detached (detach_mask=True); all ones before the first prediction, i.e. no mask
        mk = mask.detach().contiguous().view(N * hh * ww) if masked and mask is not None else None
        with torch.no_grad():  # flow is detached every iteration (detach_flow=True)
            f2 = torch.empty(N * hh * ww, 2, device=depth.device, dtype=dt)
            if dec.mask_flow and mk is not None:  # f2m = f2 · mask in the same launch
                f2m = torch.empty_like(f2)
                ops.flow_downsample(flow_full.contiguous(), Chan.whole(f2), hh, ww, 1.0 / scale,
                                    mask=mk, outm=Chan.whole(f2m))
            else:
                f2m = f2
                ops.flow_downsample(flow_full.contiguous(), Chan.whole(f2), hh, ww, 1.0 / scale)
        f2 = f2.view(N, hh, ww, 2)
        f2m = f2m.view(N, hh, ww, 2)  # the flow branch's input and the motion features' flow
        if dec.mask_corr and mk is not None:
            corr = corr_lookup(pyr, f2, N, hh, ww, L, r, mask=mk)
        else:
            corr = corr_lookup(pyr, f2, N, hh, ww, L, r)
        motion = torch.cat([_motion_features(enc, corr, f2m), f2m], -1)
        h = _gru_iteration(h, motion, it_w, ctx_pre, hc)
        fh, mh = _hidden_heads(h, [dec.flow_pred, dec.mask_pred])
        dflow = _conv(fh, dec.flow_pred.predict_layer)
        pl = dec.mask_pred.predict_layer
        mask = conv2d_nhwc(mh, pl.weight, pl.bias, 1, pl.padding, act="Sigmoid")
        dff = dflow
        for m in dec.delta_flow_encoder:
            dff = _cm(dff, m)
        mf = mask
        for m in dec.mask_encoder:
            mf = _cm(mf, m)
        drot, dtr = pose_head_train(dec.pose_pred, torch.cat([h, dff, mf], -1), label)
        if depth.is_cuda and _FUSED_LOSS:  # the losses upsample inside their fused kernel
            flow_pred = LowRes(f2 + dflow, float(scale))
            up_mask = LowRes(mask, 1.0)
        else:
            flow_pred = scale * upsample_bilinear_ac((f2 + dflow).permute(0, 3, 1, 2), scale)
            up_mask = upsample_bilinear_ac(mask.permute(0, 3, 1, 2), scale)
        if dec.detach_pose:
            R, t = R.detach(), t.detach()
        R, t = pose_update(drot, dtr, R, t, depth_transform=dec.depth_transform,
                           detach_depth_for_xy=dec.detach_depth_for_xy)
        with torch.no_grad():
            flow_full = torch.empty(N, 2, H, W, device=depth.device, dtype=dt)
            ops.pose_flow(R.detach().contiguous(), t.detach().contiguous(), K, points,
                          float(invalid_flow_num), out=flow_full)
        for lst, v in zip(outs, (flow_full, flow_pred, R, t, up_mask, drot, dtr)):
            lst.append(v)
    return outs


def _encode_images(refiner, batch: Dict[str, Tensor]) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Channels-last (feat_real, feat_render, tanh(h), relu(cxt)) of a batch's images: the feature
    encoder(s) on real and rendered, the context encoder on rendered."""
    real = batch["real_images"].permute(0, 2, 3, 1).contiguous()
    render = batch["render_images"].permute(0, 2, 3, 1).contiguous()
    N = real.shape[0]
    if refiner.real_encoder is refiner.render_encoder:  # shared: one batch of 2N images
        feats = encoder_train(refiner.real_encoder, torch.cat([real, render], 0))
        feat_real, feat_render = feats[:N], feats[N:]
    else:
        feat_real = encoder_train(refiner.real_encoder, real)
        feat_render = encoder_train(refiner.render_encoder, render)
    cx = encoder_train(refiner.context, render)
    hc = refiner.h_channels
    return feat_real, feat_render, torch.tanh(cx[..., :hc]), torch.relu(cx[..., hc:])


def _gt_flow(batch: Dict[str, Tensor], max_flow: float, dt) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(gt_flow, render_mask, depth, K), no autograd: the GT flow lifts the rendered depth with the
    reference pose and projects with the GT pose (unfiltered: each caller applies its own
    filter); render_mask = depth > 0."""
    with torch.no_grad():
        depth = batch["depth"].contiguous().to(dt)
        K = batch["internel_k"].contiguous().to(dt)
        pts = ops.lift_points(depth, K, batch["ref_rotation"].contiguous().to(dt),
                              batch["ref_translation"].contiguous().to(dt))
        gt_flow = torch.empty(depth.shape[0], 2, *depth.shape[1:], device=depth.device, dtype=dt)
        ops.pose_flow(batch["gt_rotation"].contiguous().to(dt), batch["gt_translation"].contiguous().to(dt),
                      K, pts, max_flow, out=gt_flow)
        return gt_flow, (depth > 0).to(dt), depth, K


def refiner_train_forward(refiner, batch: Dict[str, Tensor], model_points: Sequence[Tensor],
                          diameters: Sequence[float], iters: int = None) -> Dict[str, Tensor]:
    """Images → losses (SCFlowRefiner.loss), autograd graph attached.  ``batch`` keys:
    render_images, real_images [N,3,S,S]; ref_rotation, ref_translation, gt_rotation,
    gt_translation, internel_k, depth, label; optional head_label (the pose head's class label,
    default label — a data-parallel shard passes the global batch's label[:1], dist.shard_batch)."""
    dec = refiner.decoder
    check_train_flags(dec)
    begin_forward()  # per-weight use counts of this pass (batched weight gradients)
    iters = int(dec.iters if iters is None else iters)
    feat_real, feat_render, h, cxt = _encode_images(refiner, batch)
    dt = batch["real_images"].dtype
    outs = decoder_train(dec, feat_render, feat_real, h, cxt, batch["ref_rotation"],
                         batch["ref_translation"], batch["depth"], batch["internel_k"],
                         batch.get("head_label", batch["label"]), iters)
    gt_flow, render_mask, _, _ = _gt_flow(batch, refiner.max_flow, dt)
    if refiner.filter_invalid_flow and "gt_masks" in batch:
        with torch.no_grad():
            gt_flow = filter_flow_by_mask(gt_flow, batch["gt_masks"], refiner.max_flow)
    lp, lf, lm = refine_losses(outs, batch["gt_rotation"].to(dt), batch["gt_translation"].to(dt),
                               gt_flow, render_mask, batch["label"], model_points, diameters,
                               refiner.max_flow)
    return dict(loss=lp + lf + lm, loss_pose=lp, loss_flow=lf, loss_mask=lm, outs=outs, gt_flow=gt_flow)


# ------------------------------------------------------------------------------- RAFT baseline
def raft_decoder_train(dec, feat_render: Tensor, feat_real: Tensor, h: Tensor, cxt: Tensor,
                       iters: int, init_flow: Tensor = None
                       ) -> Tuple[List[Tensor], List[Tensor], List[Tensor]]:
    """RAFTDecoder.forward (raft_decoder.py:418-457) / RAFTDecoderMask.forward
    (raft_decoder_mask.py:163-208) with autograd; features, h, cxt and ``init_flow`` channels-last
    [N, h, w, C].  Returns (×8 flows [N, 2, 8h, 8w], ×8 occlusions [N, 1, 8h, 8w] — empty without
    the occlusion head —, low-resolution flows [N, h, w, 2] after every iteration).  The flow is
    detached at the top of every iteration, so its only gradient path is flow + Δflow → the
    upsampling."""
    if not dec.corr_lookup.align_corners:
        raise NotImplementedError("RAFT training: corr_lookup align_corners=True only")
    N, hh, ww, _ = feat_render.shape
    L, r = dec.num_levels, dec.radius
    scale = 2 ** (L - 1)
    convex = bool(dec.convex_upsample_flow)
    with_occ = hasattr(dec, "occlusion_pred")
    if convex and (scale != 8 or 2 * r + 1 != 9):
        raise NotImplementedError("convex upsampling: scale 8 (num_levels 4) and a 3×3 "
                                  "neighbourhood (radius 4) only")
    pyr = corr_pyramid(feat_render.permute(0, 3, 1, 2), feat_real.permute(0, 3, 1, 2), L)
    enc = dec.encoder
    hc, cc = dec.h_channels, dec.cxt_channels
    it_w, ctx_pre = _hoist_context(dec.gru, cxt, hc, cc)
    heads = [dec.flow_pred] + ([dec.mask_pred] if convex else []) + \
        ([dec.occlusion_pred] if with_occ else [])
    flow = init_flow if init_flow is not None else feat_render.new_zeros(N, hh, ww, 2)
    upflows, upoccs, lr_flows = [], [], []
    for _ in range(iters):
        flow = flow.detach()
        corr = corr_lookup(pyr, flow, N, hh, ww, L, r)
        motion = torch.cat([_motion_features(enc, corr, flow), flow], -1)
        h = _gru_iteration(h, motion, it_w, ctx_pre, hc)
        hid = _hidden_heads(h, heads)
        flow = flow + _conv(hid[0], dec.flow_pred.predict_layer)
        lr_flows.append(flow)
        occ = None
        if with_occ:  # 1×1 predictor, then the sigmoid (raft_decoder_mask.py:192-193)
            pl = dec.occlusion_pred.predict_layer
            occ = conv2d_nhwc(hid[-1], pl.weight, pl.bias, 1, pl.padding, act="Sigmoid")
        if convex:  # raw logits; the reference's `.25 *` is the op's logit_scale
            logits = _conv(hid[1], dec.mask_pred.predict_layer)
            up, upo = convex_upsample(flow, logits, occ, 0.25, float(scale))
        else:  # the reference's `mask is None` branch: bilinear, the occlusion unscaled
            up = scale * upsample_bilinear_ac(flow.permute(0, 3, 1, 2), scale)
            upo = None if occ is None else upsample_bilinear_ac(occ.permute(0, 3, 1, 2), scale)
        upflows.append(up)
        if upo is not None:
            upoccs.append(upo)
    return upflows, upoccs, lr_flows


def _sequence_loss_cfg(cfg, func: str, what: str) -> Dict[str, float]:
    """gamma / loss_weight / max_flow of a ``SequenceLoss`` over ``func`` (models/loss/
    sequence_loss.py), the reference's defaults filled in; anything else is refused."""
    if not isinstance(cfg, dict) or cfg.get("type") != "SequenceLoss":
        raise NotImplementedError(f"RAFT training: {what} must be a SequenceLoss config, got {cfg!r}")
    fc = cfg.get("loss_func_cfg")
    if not isinstance(fc, dict) or fc.get("type") != func:
        raise NotImplementedError(f"RAFT training: {what} must wrap {func}, got {fc!r}")
    known = {"type", "loss_weight", "eps"} | ({"max_flow"} if func == "RAFTLoss" else set())
    if set(fc) - known or set(cfg) - {"type", "gamma", "loss_func_cfg"}:
        raise NotImplementedError(f"RAFT training: unknown keys in {what}: {cfg!r}")
    return dict(gamma=float(cfg.get("gamma", 0.8)), weight=float(fc.get("loss_weight", 1.0)),
                max_flow=float(fc.get("max_flow", 400)), eps=float(fc.get("eps", 1e-10)))


def raft_loss_terms(refiner) -> Tuple[Dict[str, float], Optional[Dict[str, float]]]:
    """(flow loss terms, occlusion loss terms or None) from the refiner's stored loss configs:
    ``flow_loss_cfg`` + ``occlusion_loss_cfg`` (RAFTRefinerFlowMask) or ``loss_cfg``
    (RAFTRefinerFlow).  Raises NotImplementedError for what the training path does not restate."""
    if getattr(refiner, "filter_invalid_flow_by_depth", False):
        raise NotImplementedError("RAFT training: filter_invalid_flow_by_depth is not supported "
                                  "(it needs the GT pose's rendered depth)")
    if hasattr(refiner, "flow_loss_cfg"):
        return (_sequence_loss_cfg(refiner.flow_loss_cfg, "RAFTLoss", "flow_loss_cfg"),
                _sequence_loss_cfg(refiner.occlusion_loss_cfg, "L1Loss", "occlusion_loss_cfg"))
    return _sequence_loss_cfg(refiner.loss_cfg, "RAFTLoss", "loss_cfg"), None


def raft_refiner_train_forward(refiner, batch: Dict[str, Tensor], iters: int = None
                               ) -> Dict[str, Tensor]:
    """Images → losses of the RAFT baseline, autograd graph attached: RAFTRefinerFlowMask.loss
    (raft_refiner_flow_mask.py:167-220) — SequenceLoss(RAFTLoss) on the ×8 flows plus
    SequenceLoss(L1Loss) on the ×8 occlusions against ``gt_flow.sum(1) < max_flow`` — and
    RAFTRefinerFlow.loss.  The latter cannot run as the reference writes it (it unpacks
    ``get_flow``'s list of flows into three names, raft_refiner_flow.py:184); its evident intent,
    the flow sequence loss alone, is what runs here (loss_occ None, seq_occ_losses empty).
    ``batch``: the keys of ``synthetic.make_train_batch`` (no label, model points or diameters are
    needed).  Returns dict(loss, loss_flow, loss_occ, seq_flow_losses, seq_occ_losses, outs,
    gt_flow); ``outs`` = raft_decoder_train's three lists."""
    dec = refiner.decoder
    f_cfg, o_cfg = raft_loss_terms(refiner)  # refusals before any device work
    if (o_cfg is not None) != hasattr(dec, "occlusion_pred"):
        raise NotImplementedError("RAFT training: an occlusion loss needs RAFTDecoderMask, and "
                                  "RAFTDecoderMask an occlusion loss")
    begin_forward()
    iters = int(dec.iters if iters is None else iters)
    feat_real, feat_render, h, cxt = _encode_images(refiner, batch)
    dt = batch["real_images"].dtype
    outs = raft_decoder_train(dec, feat_render, feat_real, h, cxt, iters)
    upflows, upoccs, _ = outs
    max_flow = float(refiner.max_flow)
    gt_flow, render_mask, _, _ = _gt_flow(batch, max_flow, dt)
    with torch.no_grad():
        if refiner.filter_invalid_flow_by_mask:
            gt_flow = filter_flow_by_mask(gt_flow, batch["gt_masks"], max_flow)
        v = flow_valid(gt_flow, render_mask, f_cfg["max_flow"])  # iteration-invariant
        gt_occ = (gt_flow.sum(dim=1) < max_flow).to(dt)  # the reference's sum, not the magnitude
    seq_f = [flow_l1_loss(f, gt_flow, render_mask, f_cfg["max_flow"], f_cfg["weight"], f_cfg["eps"], v=v)
             for f in upflows]
    loss_flow = sequence_loss(seq_f, f_cfg["gamma"])
    seq_o, loss_occ, loss = [], None, loss_flow
    if o_cfg is not None:
        seq_o = [mask_l1_loss(o[:, 0], gt_occ, o_cfg["weight"]) for o in upoccs]
        loss_occ = sequence_loss(seq_o, o_cfg["gamma"])
        loss = loss_flow + loss_occ
    return dict(loss=loss, loss_flow=loss_flow, loss_occ=loss_occ, seq_flow_losses=seq_f,
                seq_occ_losses=seq_o, outs=outs, gt_flow=gt_flow)
