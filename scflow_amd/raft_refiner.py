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

Not covered: ``solve_pose`` / PnP (needs cv2), the data formatting (``forward_single_view``,
``format_data_*``: ``loss`` takes an already formatted batch), ``filter_invalid_flow_by_depth``
and graph-mode training — ``forward`` is ``get_flow``.
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
