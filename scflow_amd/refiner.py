"""SCFlowRefiner — the inference data flow around the decoder, on the HIP encoders + decoder.

Reference: ``models/refiner/scflow_refiner.py`` — ``__init__`` :17-63 (the feature encoder is
shared by the real and rendered images unless ``seperate_encoder``, base_refiner.py:33-40;
the context encoder is separate), ``extract_feat`` :84-106, ``get_pose`` :108-138.

Also here: the renderer-driven inference loop of ``BaseRefiner`` (base_refiner.py: the render
step of ``format_data_test`` :106-117, ``update_data`` :239-252, ``forward_multiple_pass``
:301-312, test cycles from ``test_cfg['cycles']``) as ``render`` / ``refine`` when a
``renderer`` config is given (the HIP renderer, scflow_amd/renderer.py; with ``mesh_ext='obj'``
or textured ``meshes=`` it renders UV-textured images, and ``render`` / ``refine`` /
``refine_frames`` take no argument for that).  Data loading /
pre-processing stay the reference's; the loss configuration arguments are accepted and the
losses live in ``scflow_amd.train``.

``val_step(batch)`` validates the flow of an already formatted batch on the device (end-point error
and 1 / 3 / 5 px accuracies of the flow head's and the pose-induced flow against the GT flow,
``scflow_amd/flow_eval.py``); the reference's SCFlowRefiner has none.

``get_pose`` runs the work MI355X-first rather than call by call:

* the shared feature encoder runs ONCE on cat[real, rendered] (2B images; InstanceNorm is per
  image, so batching is exact) and writes channels-last features;
* the context encoder writes tanh(h) | relu(cxt) — the split activation fused into its last
  conv — straight into the decoder's channels-last GRU working buffer;
* the decoder then runs with that buffer (no NCHW round trip for h / cxt).

``_RefinerBase`` holds what this refiner shares with the RAFT baseline's (``raft_refiner.py``):
the encoder / decoder / context construction, ``freeze_bn``, ``extract_feat`` and the fused path up
to the decoder call (``_features_into_hx``).
"""
from __future__ import annotations

import contextlib
from typing import Dict, Optional, Tuple, Union

import torch
import torch.nn as nn

from . import ops
from ._lib import ScflowError
from .encoder import RAFTEncoder
from .registry import MODELS

Tensor = torch.Tensor


def _build(cfg):
    if isinstance(cfg, nn.Module):
        return cfg
    return MODELS.build(cfg)


class _RefinerBase(nn.Module):
    """The encoders, the context encoder and the decoder of a refiner, and the two ways images
    reach the decoder: ``extract_feat`` (the reference's NCHW tensors) and ``_features_into_hx``
    (channels-last, straight into the decoder's GRU buffer)."""

    def __init__(self, seperate_encoder: bool, cxt_channels: int, h_channels: int, cxt_encoder,
                 encoder, decoder, freeze_bn: bool) -> None:
        super().__init__()
        self.seperate_encoder = seperate_encoder
        if seperate_encoder:
            self.render_encoder = _build(encoder)
            self.real_encoder = _build(encoder)
        else:
            enc = _build(encoder)
            self.render_encoder = enc
            self.real_encoder = enc
        self.decoder = _build(decoder)
        self.context = _build(cxt_encoder)
        self.h_channels, self.cxt_channels = h_channels, cxt_channels
        assert self.h_channels == self.decoder.h_channels
        assert self.cxt_channels == self.decoder.cxt_channels
        assert self.h_channels + self.cxt_channels == self.context.out_channels
        # scflow_refiner.py:58-61.  The flag is kept and re-applied by train(): the reference
        # applies it once in __init__, so mmengine's later model.train() puts its BatchNorms
        # back in train mode; here a frozen module stays frozen.
        self.freeze_bn_flag = bool(freeze_bn)
        if freeze_bn:
            self.freeze_bn()
        # opt-in bf16 direct conv for the encoders' stride-1 3×3 convs (RAFTEncoder.bf16, DESIGN.md
        # §26): re-read at every extract_feat / fused forward, independent of the decoder's
        # gru_bf16 / menc_bf16; inference only
        self.enc_bf16 = False

    def _set_enc_bf16(self) -> None:
        for enc in (self.real_encoder, self.render_encoder, self.context):
            enc.bf16 = bool(self.enc_bf16)

    def freeze_bn(self) -> None:
        """scflow_refiner.py:75-78, raft_refiner_flow.py:75-78: every BatchNorm2d in eval mode
        (running statistics, no update); its affine parameters stay trainable."""
        self.freeze_bn_flag = True
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()

    def train(self, mode: bool = True):
        super().train(mode)
        if mode and self.freeze_bn_flag:
            self.freeze_bn()
        return self

    @contextlib.contextmanager
    def _eval_mode(self):
        """Every module in eval mode inside the block (the HIP encoders run BatchNorm on its
        running statistics only), each module's own flag put back afterwards."""
        modes = [(m, m.training) for m in self.modules()]
        self.eval()
        try:
            yield
        finally:
            for m, t in modes:
                m.training = t

    def extract_feat(self, render_images: Tensor, real_images: Tensor
                     ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        """scflow_refiner.py:84-106, raft_refiner_flow.py:90-113 — NCHW (render_feat, real_feat,
        tanh(h), relu(cxt))."""
        self._set_enc_bf16()
        real_feat = self.real_encoder(real_images)
        render_feat = self.render_encoder(render_images)
        n = render_images.shape[0]
        c = self.context.forward_cl(render_images.contiguous().float(), act="Tanh", act2="ReLU",
                                    act_split=self.h_channels)
        _, h, w, _ = c.shape
        h_feat = ops.chan_to_nchw(ops.Chan(c, 0, self.h_channels), n, h, w)
        cxt_feat = ops.chan_to_nchw(ops.Chan(c, self.h_channels, self.cxt_channels), n, h, w)
        return render_feat, real_feat, h_feat, cxt_feat

    def _features_into_hx(self, render: Tensor, real: Tensor):
        """The fused path up to the decoder call: (render_feat, real_feat, hx, h, w) with ``hx``
        the decoder's channels-last GRU buffer, tanh(h) | relu(cxt) already in place."""
        N = real.shape[0]
        self._set_enc_bf16()
        # feature encoder(s): one launch sequence over cat[real, render] when shared
        if self.real_encoder is self.render_encoder:
            both = torch.cat([real, render], 0)
            fcl = self.real_encoder.forward_cl(both)
            n2, h, w, _ = fcl.shape
            feats = ops.chan_to_nchw(ops.Chan.whole(fcl), n2, h, w)
            real_feat, render_feat = feats[:N], feats[N:]
        else:
            real_feat = self.real_encoder(real)
            render_feat = self.render_encoder(render)
            h, w = real_feat.shape[-2:]
        # context encoder → tanh(h) | relu(cxt) straight into the decoder's GRU buffer
        hx_c = self.decoder.hx_channels
        hx = torch.empty(N * h * w, hx_c, device=real.device)
        self.context.forward_cl(render, out=hx.view(N, h, w, hx_c), act="Tanh", act2="ReLU",
                                act_split=self.h_channels)
        return render_feat.contiguous(), real_feat.contiguous(), hx, h, w


@MODELS.register_module()
class SCFlowRefiner(_RefinerBase):
    def __init__(self, cxt_channels: int, h_channels: int, seperate_encoder: bool, cxt_encoder: dict,
                 encoder: dict, decoder: dict, renderer=None, render_augmentations=None,
                 pose_loss_cfg=None, flow_loss_cfg=None, mask_loss_cfg=None, max_flow: float = 400.,
                 filter_invalid_flow: bool = True, freeze_encoder: bool = False,
                 freeze_bn: bool = False, train_cfg: Optional[dict] = None,
                 test_cfg: Optional[dict] = None, init_cfg=None) -> None:
        super().__init__(seperate_encoder, cxt_channels, h_channels, cxt_encoder, encoder, decoder,
                         freeze_bn)
        self.max_flow = max_flow
        self.filter_invalid_flow = filter_invalid_flow
        self.train_cfg = train_cfg or {}
        self.test_cfg = test_cfg or {}
        self.test_iter_num = self.test_cfg.get("iters", self.decoder.iters)
        self.test_cycle_num = self.test_cfg.get("cycles", 1)
        self.renderer = None
        if renderer is not None:
            from .renderer import Renderer
            self.renderer = renderer if isinstance(renderer, Renderer) else Renderer(**renderer)
        # scflow_refiner.py:58-61; kept and re-applied by train() like freeze_bn
        # (requires_grad=False persists in both)
        self.freeze_encoder_flag = bool(freeze_encoder)
        if freeze_encoder:
            self.freeze_encoder()

    def freeze_encoder(self) -> None:
        """scflow_refiner.py:65-73: the feature encoders (real and rendered; one module when
        shared) in eval mode with requires_grad=False.  The context encoder stays trainable."""
        self.freeze_encoder_flag = True
        for enc in (self.real_encoder, self.render_encoder):
            for m in enc.modules():
                m.eval()
                for p in m.parameters():
                    p.requires_grad = False

    def train(self, mode: bool = True):
        super().train(mode)
        if mode and self.freeze_encoder_flag:
            for enc in (self.real_encoder, self.render_encoder):
                enc.eval()
        return self

    def to(self, *args, **kwargs):  # base_refiner.py:69-72: the renderer's meshes move too
        if self.renderer is not None:
            dev = args[0] if args else kwargs.get("device")
            if dev is not None and not isinstance(dev, torch.dtype):
                self.renderer.to(dev)
        return super().to(*args, **kwargs)

    def cuda(self, device=None):
        if self.renderer is not None:
            self.renderer.to("cuda" if device is None else torch.device("cuda", device))
        return super().cuda(device)

    # ------------------------------------------------------------------ renderer-driven loop
    def render(self, rotations: Tensor, translations: Tensor, internel_k: Tensor, labels: Tensor,
               norm_mean=(0.0, 0.0, 0.0), norm_std=(255.0, 255.0, 255.0)):
        """format_data_test's render step (base_refiner.py:106-117): rendered images (RGB,
        normalised with img_norm_cfg /255 — mean 0 / std 255 in the config, i.e. identity),
        rendered depth (zbuf), rendered masks (depth > 0)."""
        if self.renderer is None:
            raise RuntimeError("SCFlowRefiner was built without a renderer config")
        out = self.renderer(rotations, translations, internel_k, labels)
        img = out["images"][..., :3].permute(0, 3, 1, 2).contiguous()
        mean = torch.tensor(norm_mean, device=img.device).view(1, 3, 1, 1) / 255.0
        std = torch.tensor(norm_std, device=img.device).view(1, 3, 1, 1) / 255.0
        img = (img - mean) / std
        depth = out["fragments"].zbuf[..., 0]
        return img, depth, (depth > 0).float()

    def refine(self, real_images: Tensor, ref_rotations: Tensor, ref_translations: Tensor,
               internel_k: Tensor, labels: Tensor, cycles: Optional[int] = None):
        """Test-time refinement (base_refiner.py:301-312 + scflow_refiner.py:142-177): for each
        cycle render the current pose, run ``get_pose`` with ``test_cfg['iters']`` iterations and
        take the last pose; returns (rotations, translations, last get_pose outputs)."""
        cycles = self.test_cycle_num if cycles is None else cycles
        R, t = ref_rotations, ref_translations
        iters = self.decoder.iters
        self.decoder.iters = self.test_iter_num
        try:
            for _ in range(cycles):
                img, depth, _ = self.render(R, t, internel_k, labels)
                out = self.get_pose(img, real_images, R, t, depth, internel_k, labels)
                R, t = out[2][-1], out[3][-1]
        finally:
            self.decoder.iters = iters
        return R, t, out

    def refine_frames(self, frames: Tensor, frame_index: Tensor, ref_rotations: Tensor,
                      ref_translations: Tensor, ori_k: Tensor, labels: Tensor,
                      cycles: Optional[int] = None, points=None):
        """Decoded frames [F, H, W, 3] uint8 plus N detections (frame_index, reference poses,
        ori_k per object or per frame, labels) → poses in the ORIGINAL camera:
        ``patches.frames_to_patches`` (crop, resize, pad and the adapted intrinsics on the device,
        at the renderer's image size) and then ``refine`` on its patches and ``internel_k`` —
        with the intrinsics adapted the crop leaves the pose as it is (pose.py:275-277).  Returns
        (rotations, translations, valid, data): where ``valid`` is False the pose is the input
        pose; ``data`` is ``frames_to_patches``' dict.  ``points``: a (points, counts) table,
        default ``patches.point_table`` of the renderer's meshes (built once)."""
        from . import patches
        if self.renderer is None:
            raise RuntimeError("SCFlowRefiner was built without a renderer config")
        if points is None:
            if getattr(self, "_point_table", None) is None or \
                    self._point_table[0].device != self.renderer._device:
                self._point_table = patches.point_table(self.renderer)
            points = self._point_table
        data = patches.frames_to_patches(frames, frame_index, ref_rotations, ref_translations,
                                         ori_k, labels, points[0], points[1],
                                         size=self.renderer.image_size[0])
        R, t, _ = self.refine(data["real_images"], ref_rotations, ref_translations,
                              data["internel_k"], labels, cycles=cycles)
        valid = data["valid"]
        R = torch.where(valid.view(-1, 1, 1), R, ref_rotations)
        t = torch.where(valid.view(-1, 1), t, ref_translations)
        return R, t, valid, data

    def train_batch_from_frames(self, frames: Tensor, masks: Tensor, frame_index: Tensor,
                                gt_rotations: Tensor, gt_translations: Tensor, ori_k: Tensor,
                                labels: Tensor, diameters: Tensor, seed: int, step: int,
                                aug: Optional[dict] = None, object_offset: int = 0,
                                drop_invalid: bool = False, points=None, *,
                                backgrounds: Optional[Tensor] = None,
                                background_sizes: Optional[Tensor] = None,
                                background_p: float = 0.3,
                                background_index: Optional[Tensor] = None) -> Dict[str, Tensor]:
        """Decoded frames [F, H, W, 3] uint8, instance masks [F, H, W] uint8 and N annotated
        objects → the batch ``train.step.TrainStep`` takes: ``patches.frames_to_train_patches``
        (pose jitter, random crop, colour augmentation, all on the device, at the renderer's image
        size) plus ``render_images`` and ``depth`` rendered at the jittered pose under
        ``internel_k`` — format_data_train_sup (base_refiner.py:154-225).  ``diameters`` [C]
        float32; ``points`` as in ``refine_frames``.  The default keeps all N objects and
        synchronises nothing (``valid`` says which are usable); ``drop_invalid=True`` compacts
        every per-object entry by ``valid``, which costs ONE host synchronisation (the number of
        valid objects sizes the result).  ``backgrounds`` and the other ``background_*``
        keywords: ``frames_to_train_patches``' (RandomBackground; the batch gains
        ``background_index``)."""
        from . import patches
        if self.renderer is None:
            raise RuntimeError("SCFlowRefiner was built without a renderer config")
        if points is None:
            if getattr(self, "_point_table", None) is None or \
                    self._point_table[0].device != self.renderer._device:
                self._point_table = patches.point_table(self.renderer)
            points = self._point_table
        data = patches.frames_to_train_patches(
            frames, masks, frame_index, gt_rotations, gt_translations, ori_k, labels, points[0],
            points[1], diameters, seed, step, aug=aug, size=self.renderer.image_size[0],
            object_offset=object_offset, backgrounds=backgrounds,
            background_sizes=background_sizes, background_p=background_p,
            background_index=background_index)
        if drop_invalid:
            keep = data["valid"].nonzero()[:, 0]  # the synchronisation
            data = {k: v[keep] for k, v in data.items()}
        img, depth, _ = self.render(data["ref_rotation"], data["ref_translation"],
                                    data["internel_k"], data["label"])
        data["render_images"], data["depth"] = img, depth
        return data

    # ------------------------------------------------------------------ reference API
    def get_pose(self, render_images: Tensor, real_images: Tensor, ref_rotation: Tensor,
                 ref_translation: Tensor, depth: Tensor, internel_k: Tensor, label: Tensor,
                 init_flow: Optional[Tensor] = None, head_label: Optional[Tensor] = None):
        """scflow_refiner.py:108-138 — images → encoders → SCFlowDecoder outputs (7 lists)."""
        if render_images.device.type != "cuda":
            raise ScflowError("SCFlowRefiner runs on the gfx950 HIP kernels only (no CPU fallback)")
        with torch.no_grad():
            return self._get_pose(render_images.contiguous().float(), real_images.contiguous().float(),
                                  ref_rotation, ref_translation, depth, internel_k, label, init_flow,
                                  head_label)

    def forward(self, *args, **kwargs):
        return self.get_pose(*args, **kwargs)

    def val_step(self, batch):
        """Flow validation on an already formatted batch (the keys ``loss`` / ``TrainStep`` take,
        ``synthetic.make_train_batch``; ``gt_masks`` optional): ``get_pose`` at
        ``test_cfg['iters']`` iterations under ``no_grad``, then the end-point error of the last
        flow from the flow head against the GT flow — ``epe_mean``, ``epe_1px``, ``epe_3px``,
        ``epe_5px`` and, with ``gt_masks``, ``epe_noc_*`` (the keys of RAFTRefinerFlowMask's
        ``val_step``, raft_refiner_flow_mask.py:239-281, ``reduction='total_mean'``) — and the same
        for the last pose-induced flow as ``pose_epe_*`` / ``pose_epe_noc_*``.  The reference's
        SCFlowRefiner has no ``val_step``: this is an extension.  → ``dict(log_vars, num_samples)``;
        one ``scflow_flow_gt`` launch serves both flows, and the one host synchronisation is where
        ``log_vars`` turns into floats.  The forward runs in eval mode; ``decoder.iters`` and every
        module's training mode are left as they were."""
        from . import flow_eval
        iters, self.decoder.iters = self.decoder.iters, self.test_iter_num
        try:
            with self._eval_mode():
                out = self.get_pose(batch["render_images"], batch["real_images"],
                                    batch["ref_rotation"], batch["ref_translation"], batch["depth"],
                                    batch["internel_k"], batch["label"])
        finally:
            self.decoder.iters = iters
        with torch.no_grad():
            masks = batch.get("gt_masks")
            flow, noc = flow_eval.gt_flow(batch["depth"], batch["internel_k"], batch["ref_rotation"],
                                          batch["ref_translation"], batch["gt_rotation"],
                                          batch["gt_translation"], invalid_num=self.max_flow,
                                          gt_mask=masks)
            noc = noc if masks is not None else None
            metric = flow_eval.epe_and_occ_against(flow, noc, out[1][-1], None, self.max_flow,
                                                   "total_mean")
            metric.update(flow_eval.epe_and_occ_against(flow, noc, out[0][-1], None, self.max_flow,
                                                        "total_mean", prefix="pose_epe"))
            return dict(log_vars=flow_eval.log_vars(metric), num_samples=len(out[1][-1]))

    # ------------------------------------------------------------------ fused path
    def _get_pose(self, render, real, R, t, depth, K, label, init_flow, head_label=None):
        N, _, H, W = real.shape
        render_feat, real_feat, hx, _, _ = self._features_into_hx(render, real)
        if init_flow is None:
            init_flow = torch.zeros(N, 2, H, W, device=real.device)
        return self.decoder._forward(render_feat, real_feat, None, None, R, t, depth, K, label,
                                     init_flow, 0.0, hx=hx, head_label=head_label)
