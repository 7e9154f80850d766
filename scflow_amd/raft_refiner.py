"""RAFTRefinerFlow / RAFTRefinerFlowMask — the flow half of the reference's RAFT + PnP baseline,
on the HIP encoders and the HIP RAFT decoders.

Reference: ``models/refiner/raft_refiner_flow.py`` (``__init__`` :30-72, ``extract_feat`` :90-113,
``get_flow`` :115-137) and ``models/refiner/raft_refiner_flow_mask.py`` (``__init__`` :34-79,
``extract_feat`` :86-116, ``get_flow`` :118-130); the encoders are shared by the real and the
rendered images unless ``seperate_encoder`` (base_refiner.py:33-40), the context encoder is
separate.  The loss configurations are accepted and kept, as ``SCFlowRefiner`` keeps them.

``get_flow`` takes ``SCFlowRefiner._get_pose``'s device-side path (``refiner.py``'s
``_RefinerBase._features_into_hx``, which also holds the construction, ``freeze_bn`` and
``extract_feat``): the shared feature encoder runs ONCE over cat[real, rendered], the context
encoder writes tanh(h) | relu(cxt) straight into the decoder's channels-last GRU working buffer,
and the decoder runs with that buffer.  It returns
the decoder's lists (``upflow_preds``; with the mask decoder ``(upflow_preds,
upocclusion_preds)``).

``loss(batch)`` is the reference's training loss (``SequenceLoss(RAFTLoss)`` on the ×8 flows plus,
with the mask decoder, ``SequenceLoss(L1Loss)`` on the ×8 occlusions) on the HIP autograd
Functions, convex upsampling included (``scflow_convex_upsample_bwd``); ``train.step.TrainStep``
takes these refiners.  The inference paths above stay under ``torch.no_grad()``.

``val_step(batch)`` (raft_refiner_flow_mask.py:261-281) validates the flow: ``get_flow`` at
``test_cfg['iters']``, then the end-point error, its 1 / 3 / 5 px accuracies and the occlusion error
against the GT flow on the device (``scflow_amd/flow_eval.py``).

``solve_pose`` (base_flow_refiner.py:99-155) and ``get_pose`` turn the last ×8 flow into poses on
the batched HIP RANSAC-PnP (``ops.pnp_ransac``: compacted 2D-3D correspondences, P3P hypotheses on
hashed samples, one scoring kernel, Gauss-Newton on the winner's inliers) instead
of ``cv2.solvePnPRansac`` per sample behind ``.cpu().numpy()`` (pose.py:203-249).  It takes the
reference's parameters (``occ_thresh``, ``sample_points``, ``solve_pose_param``) and returns its
dict, but it is another algorithm: parity with cv2 is unpinned (cv2 is absent here).  Everything
stays on the device; ``solve_pose``'s one host synchronisation is the final dropping of failed
samples.  ``solve_pose_mode='progressive-x'`` and ``solve_pose_space='origin'`` raise.

Not covered: the data formatting (``forward_single_view``, ``format_data_*``: ``loss`` takes an
already formatted batch), ``remap_pose_to_origin_resoluaion``, ``filter_invalid_flow_by_depth`` and
graph-mode training — ``forward`` is ``get_flow``.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional, Sequence

import torch

from ._lib import ScflowError
from .refiner import _RefinerBase
from .registry import MODELS

Tensor = torch.Tensor


class _RAFTFlowRefiner(_RefinerBase):
    """What the two RAFT refiners add to the shared base (BaseFlowRefiner's constructor
    arguments, ``get_flow`` and ``loss``)."""

    def __init__(self, seperate_encoder: bool, cxt_channels: int, h_channels: int, cxt_encoder: dict,
                 encoder: dict, decoder: dict, renderer: Optional[dict], max_flow: float,
                 render_augmentations: Optional[Sequence], filter_invalid_flow_by_mask: bool,
                 filter_invalid_flow_by_depth: bool, freeze_bn: bool, train_cfg: Optional[dict],
                 test_cfg: Optional[dict], init_cfg) -> None:
        super().__init__(seperate_encoder, cxt_channels, h_channels, cxt_encoder, encoder, decoder,
                         freeze_bn)
        self.max_flow = max_flow
        self.filter_invalid_flow_by_mask = filter_invalid_flow_by_mask
        self.filter_invalid_flow_by_depth = filter_invalid_flow_by_depth
        self.renderer_cfg = renderer
        self.render_augmentations = render_augmentations
        self.train_cfg = train_cfg or {}
        self.test_cfg = test_cfg or {}
        self.init_cfg = init_cfg
        self.test_iter_num = self.test_cfg.get("iters") if "iters" in self.test_cfg \
            else self.decoder.iters

    # ------------------------------------------------------------------ reference API
    def get_flow(self, render_images: Tensor, real_images: Tensor,
                 init_flow: Optional[Tensor] = None):
        """raft_refiner_flow.py:115-137 — images → encoders → the RAFT decoder's lists.
        ``init_flow`` [B, 2, H/8, W/8] is at the feature resolution (zeros when None)."""
        if render_images.device.type != "cuda":
            raise ScflowError(f"{type(self).__name__} runs on the gfx950 HIP kernels only (no CPU "
                              "fallback)")
        with torch.no_grad():
            return self._get_flow(render_images.contiguous().float(),
                                  real_images.contiguous().float(), init_flow)

    def forward(self, *args, **kwargs):
        return self.get_flow(*args, **kwargs)

    def loss(self, batch):
        """raft_refiner_flow_mask.py:167-220 / raft_refiner_flow.py ``loss`` on an already
        formatted batch (the keys of ``synthetic.make_train_batch``): the training forward on the
        HIP autograd Functions (train/model.py ``raft_refiner_train_forward``) → ``(loss, None,
        log_vars)`` with the reference's ``log_vars`` keys (``seq_{i}_flow_loss``,
        ``seq_{i}_occ_loss``, ``loss_occ``, ``loss_flow``, ``loss``), fetched with one host
        synchronisation.  ``loss`` carries the autograd graph.  RAFTRefinerFlow has no occlusion
        terms (see ``raft_refiner_train_forward`` on the reference's own ``loss``)."""
        from .train.model import raft_loss_terms, raft_refiner_train_forward
        raft_loss_terms(self)  # configuration refusals come first
        if batch["render_images"].device.type != "cuda":
            raise ScflowError(f"{type(self).__name__}.loss runs on the gfx950 HIP kernels only "
                              "(no CPU fallback)")
        res = raft_refiner_train_forward(self, batch)
        seq_f, seq_o = res["seq_flow_losses"], res["seq_occ_losses"]
        names, vals = [], []
        for i, f in enumerate(seq_f):
            names.append(f"seq_{i}_flow_loss")
            vals.append(f)
            if seq_o:
                names.append(f"seq_{i}_occ_loss")
                vals.append(seq_o[i])
        if seq_o:
            names.append("loss_occ")
            vals.append(res["loss_occ"])
        names += ["loss_flow", "loss"]
        vals += [res["loss_flow"], res["loss"]]
        host = torch.stack([v.detach().reshape(()) for v in vals]).tolist()  # the one sync
        return res["loss"], None, OrderedDict(zip(names, host))

    def val_step(self, batch):
        """raft_refiner_flow_mask.py:261-281 on an already formatted batch (the keys ``loss`` takes;
        ``gt_masks`` optional): ``get_flow`` at ``test_cfg['iters']`` iterations under ``no_grad``,
        then ``flow_eval.eval_epe_and_occ(reduction='total_mean')`` of the last ×8 flow → ``dict(
        log_vars, num_samples)``.  With the mask decoder ``log_vars`` holds the reference's keys
        (``epe_*``, ``epe_noc_*`` with ``gt_masks``, ``occ`` of the last occlusion).  RAFTRefinerFlow:
        the same without ``occ``, and without ``gt_masks`` ``epe_noc_*`` repeats ``epe_*`` — the
        evident intent of BaseFlowRefiner's ``val_step`` / ``eval_epe`` (base_flow_refiner.py:74-96),
        which cannot run as written (``reducion=``, :89, and a call with one argument too many,
        :80-81).  One host synchronisation, where ``log_vars`` turns into floats; The forward
        runs in eval mode; ``decoder.iters`` and every module's training mode are left as they
        were."""
        from . import flow_eval
        iters, self.decoder.iters = self.decoder.iters, self.test_iter_num
        try:
            with self._eval_mode():
                out = self.get_flow(batch["render_images"], batch["real_images"])
        finally:
            self.decoder.iters = iters
        flows, occs = out if isinstance(out, tuple) else (out, None)
        with torch.no_grad():
            metric = flow_eval.eval_epe_and_occ(
                flows[-1], None if occs is None else occs[-1], batch["depth"], batch["gt_rotation"],
                batch["gt_translation"], batch["internel_k"], batch["ref_rotation"],
                batch["ref_translation"], batch.get("gt_masks"), max_flow=self.max_flow,
                reduction="total_mean", noc_without_mask=occs is None)
            return dict(log_vars=flow_eval.log_vars(metric), num_samples=len(flows[-1]))

    # ------------------------------------------------------------------ RANSAC-PnP
    def _pnp_valid(self, occlusion: Optional[Tensor], rendered_depths: Tensor) -> Optional[Tensor]:
        """The validity mask ``solve_pose`` hands the PnP beside ``depth > 0``: occlusion >
        ``occ_thresh`` (base_flow_refiner.py:110-114), thinned by ``sample_points``
        (:117-126) — all torch ops on the device.  None: every rendered pixel."""
        valid = None
        if occlusion is not None:
            occlusion = occlusion.reshape(rendered_depths.shape).float()
            valid = occlusion > self.test_cfg.get("occ_thresh", 0.5)
        cfg = self.test_cfg.get("sample_points", None)
        if cfg is None:
            return valid
        num, mode = int(cfg.get("num", 1000)), cfg.get("mode", "random")
        cand = rendered_depths > 0
        if valid is not None:
            cand = cand & valid
        B = cand.shape[0]
        flat = cand.reshape(B, -1)
        if mode == "random":
            # a uniform draw of `num` of the candidates (all of them when fewer): torch's generator,
            # not the reference's randperm stream, and without its never-the-last-point quirk
            key = torch.rand(flat.shape, device=flat.device)
        elif occlusion is not None:
            key = occlusion.reshape(B, -1)  # topk on the occlusion confidence (:54-63)
        else:
            raise ScflowError("sample_points mode 'topk' selects on the occlusion confidence: it "
                              "needs the mask decoder's occlusion")
        key = torch.where(flat, key.float(), key.new_full((), float("-inf"), dtype=torch.float32))
        k = min(num, flat.shape[1])
        idx = torch.topk(key, k, dim=1).indices
        keep = torch.zeros_like(flat).scatter_(1, idx, True) & flat
        return keep.reshape(cand.shape)

    def _pnp(self, flow: Tensor, rendered_depths: Tensor, ref_rotations: Tensor,
             ref_translations: Tensor, internel_k: Tensor, occlusion: Optional[Tensor]):
        cfg = self.test_cfg
        mode = cfg.get("solve_pose_mode", "ransacpnp")
        if mode != "ransacpnp":
            raise ScflowError(f"solve_pose_mode={mode!r} is not built: only 'ransacpnp' runs on the "
                              "HIP kernels ('progressive-x' needs pyprogressivex)")
        if cfg.get("solve_pose_space", "transformed") == "origin":
            raise ScflowError("solve_pose_space='origin' is not built: poses are solved in the "
                              "cropped patch's frame ('transformed')")
        if flow.device.type != "cuda":
            raise ScflowError(f"{type(self).__name__} runs on the gfx950 HIP kernels only (no CPU "
                              "fallback)")
        from .library import pnp_ransac
        param = cfg.get("solve_pose_param", {})
        valid = self._pnp_valid(occlusion, rendered_depths)
        return pnp_ransac(
            flow, rendered_depths, ref_rotations, ref_translations, internel_k,
            None if valid is None else valid.float(), int(param.get("iterationscount", 100)),
            float(param.get("reprojectionerror", 3.0)), 10, 0)

    def solve_pose(self, batch_flow: Tensor, rendered_depths: Tensor, ref_rotations: Tensor,
                   ref_translations: Tensor, internel_k: Tensor, labels: Tensor, per_img_patch_num,
                   occlusion: Optional[Tensor] = None):
        """base_flow_refiner.py:99-155 on the batched HIP RANSAC-PnP (``ops.pnp_ransac``) — the ×8
        flow [B, 2, H, W], rendered depths [B, H, W], reference poses, intrinsics, labels [B] and
        the patches per image → the reference's dict of per-image lists (``rotations``,
        ``translations``, ``scores`` = ones, ``labels``) with the samples whose PnP failed dropped.
        One host synchronisation, at the end (the boolean indexing).  ``test_cfg`` is read as the
        reference reads it: ``occ_thresh``, ``sample_points``, ``solve_pose_param``."""
        with torch.no_grad():
            R, t, ok, _ = self._pnp(batch_flow, rendered_depths, ref_rotations, ref_translations,
                                    internel_k, occlusion)
        split = [int(v) for v in per_img_patch_num]
        keep = torch.split(ok, split)
        scores = torch.ones_like(labels, dtype=torch.float32)
        out = {}
        for name, x in (("rotations", R), ("translations", t), ("scores", scores),
                        ("labels", labels)):
            out[name] = [p[k] for p, k in zip(torch.split(x, split), keep)]
        return out

    def get_pose(self, render_images: Tensor, real_images: Tensor, rendered_depths: Tensor,
                 ref_rotations: Tensor, ref_translations: Tensor, internel_k: Tensor):
        """``get_flow`` at ``test_iter_num`` iterations, then RANSAC-PnP on the last ×8 flow (with
        the mask decoder: restricted by the last occlusion) → (R [B, 3, 3], t [B, 3], ok [B] bool,
        inliers [B] int32), all on the device; the reference pose where ``ok`` is False."""
        iters, self.decoder.iters = self.decoder.iters, self.test_iter_num
        try:
            out = self.get_flow(render_images, real_images)
        finally:
            self.decoder.iters = iters
        flows, occs = out if isinstance(out, tuple) else (out, None)
        with torch.no_grad():
            return self._pnp(flows[-1], rendered_depths.contiguous().float(), ref_rotations,
                             ref_translations, internel_k, None if occs is None else occs[-1])

    # ------------------------------------------------------------------ fused path
    def _get_flow(self, render, real, init_flow):
        render_feat, real_feat, hx, h, w = self._features_into_hx(render, real)
        if init_flow is None:
            init_flow = torch.zeros(real.shape[0], 2, h, w, device=real.device)
        return self.decoder._forward(render_feat, real_feat, init_flow, None, None, hx=hx)


@MODELS.register_module()
class RAFTRefinerFlow(_RAFTFlowRefiner):
    def __init__(self, seperate_encoder: bool, cxt_channels: int, h_channels: int, cxt_encoder: dict,
                 encoder: dict, decoder: dict, renderer: Optional[dict] = None,
                 loss_cfg: Optional[dict] = None, max_flow: float = 400.,
                 render_augmentations: Optional[Sequence] = None,
                 filter_invalid_flow_by_mask: bool = True,
                 filter_invalid_flow_by_depth: bool = False, freeze_bn: bool = False,
                 train_cfg: Optional[dict] = dict(), test_cfg: Optional[dict] = dict(),
                 init_cfg=None) -> None:
        super().__init__(seperate_encoder, cxt_channels, h_channels, cxt_encoder, encoder, decoder,
                         renderer, max_flow, render_augmentations, filter_invalid_flow_by_mask,
                         filter_invalid_flow_by_depth, freeze_bn, train_cfg, test_cfg, init_cfg)
        self.loss_cfg = loss_cfg


@MODELS.register_module()
class RAFTRefinerFlowMask(_RAFTFlowRefiner):
    def __init__(self, seperate_encoder: bool, cxt_channels: int, h_channels: int, cxt_encoder: dict,
                 encoder: dict, decoder: dict, renderer: Optional[dict] = None,
                 flow_loss_cfg: Optional[dict] = None, occlusion_loss_cfg: Optional[dict] = None,
                 max_flow: float = 400., render_augmentations: Optional[list] = None,
                 filter_invalid_flow_by_mask: bool = True,
                 filter_invalid_flow_by_depth: bool = False, freeze_bn: bool = False,
                 train_cfg: Optional[dict] = dict(), test_cfg: Optional[dict] = dict(),
                 init_cfg=None) -> None:
        super().__init__(seperate_encoder, cxt_channels, h_channels, cxt_encoder, encoder, decoder,
                         renderer, max_flow, render_augmentations, filter_invalid_flow_by_mask,
                         filter_invalid_flow_by_depth, freeze_bn, train_cfg, test_cfg, init_cfg)
        self.flow_loss_cfg, self.occlusion_loss_cfg = flow_loss_cfg, occlusion_loss_cfg
        self.vis_tensorboard = False
