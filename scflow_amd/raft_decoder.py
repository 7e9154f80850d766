"""RAFTDecoder / RAFTDecoderMask — drop-in replacements for the reference's RAFT + PnP baseline
decoders, running on the gfx950 HIP kernels.

Reference: ``models/decoder/raft_decoder.py:299-457`` (``RAFTDecoder``) and
``models/decoder/raft_decoder_mask.py:21-208`` (``RAFTDecoderMask``; the shipped config is
``configs/refine_models/raft.py:40-48``, 12 iterations).  Same constructor kwargs (the misspelt
``convex_unsample_flow`` included), same submodules and state-dict keys (reference checkpoints
load with ``strict=True``), same ``forward(feat1, feat2, flow, h_feat, cxt_feat)`` and the same
returned lists.  ``iters`` is re-read on every call (the refiners overwrite it temporarily,
``raft_refiner_flow.py:146-149``).

Forward, per call (B pairs, features h×w = image/8, M = B·h·w), everything on the current stream:

* once: the correlation pyramid (tiled where the geometry allows), the channels-last working
  buffer ``HX = [h | cxt | motion | flow]`` (exactly the GRU's ``cat[h, x]``) and the context's
  loop-invariant share of the GRU pre-activations;
* ``iters`` times: lookup (fused with corr_net.0 where the shared core plans it) → motion encoder →
  GRU → the hidden convs of the two or three XHeads as ONE launch (cout 512 / 768) → the 3×3 flow
  predictor, the 1×1 mask predictor (576 logits) and the 1×1 occlusion predictor with its sigmoid
  → ``scflow_convex_upsample``: one softmax per sub-pixel serves the ×8 flow and the ×8 occlusion,
  and the same launch writes flow + Δflow into the next iteration's lookup buffer and into HX's
  flow channels.  The low-resolution flow alternates between two buffers (the launch reads its
  neighbours' pixels, so it cannot update the flow in place).

The launches whose arguments do not change between iterations are recorded once (``ops.binding``)
and replayed; no host synchronisation happens inside ``forward``.  There is no CPU path, no second
stream and no deferred full-resolution work here.  ``net_type='Small'`` is not supported.

The constructor's common part and the iteration up to the GRU (pyramid, ``HX``, lookup, motion
encoder, GRU, the recorded segments and their planning) are ``recurrent.py``'s, shared with
``SCFlowDecoder``; this file holds the head predictors and the upsampling tail.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import torch

from . import ops
from ._lib import ScflowError
from .modules import ConvRunner, XHead, run_chain
from .ops import Chan
from .recurrent import RecurrentCore, _RecurrentDecoder
from .registry import MODELS

Tensor = torch.Tensor


@MODELS.register_module()
class RAFTDecoder(_RecurrentDecoder):
    _with_occlusion = False

    def __init__(self, net_type: str, num_levels: int, radius: int, iters: int,
                 corr_lookup_cfg: dict = dict(type="CorrLookup", align_corners=True),
                 gru_type: str = "SeqConv", feat_channels: Union[int, Sequence[int]] = 256,
                 mask_channels: int = 64, convex_unsample_flow: bool = True,
                 conv_cfg: Optional[dict] = None, norm_cfg: Optional[dict] = None,
                 act_cfg: Optional[dict] = None) -> None:
        if net_type == "Small":
            raise NotImplementedError("net_type Small (82 / 96 / 64-channel tensors, no mask "
                                      "predictor) is not supported by the HIP RAFT decoders")
        super().__init__(net_type, num_levels, radius, iters, corr_lookup_cfg, gru_type,
                         feat_channels, conv_cfg, norm_cfg, act_cfg)
        # raft_decoder.py:356: the 3×3 neighbourhood's 9 taps are spelt 2·radius + 1
        self.mask_channels = mask_channels * (2 * radius + 1)
        self.flow_pred = XHead(self.h_channels, self.feat_channels, 2, x="flow")
        if self._with_occlusion:
            self.occlusion_pred = XHead(self.h_channels, self.feat_channels, 1, x="mask")
        self.mask_pred = XHead(self.h_channels, self.feat_channels, self.mask_channels, x="mask")
        self.convex_upsample_flow = convex_unsample_flow
        # also keep the low-resolution flow after every iteration (flow + Δflow, NCHW) in
        # ``lr_flows``: one transpose launch per iteration; for tests and warm starts
        self.keep_lr_flows = False
        self.lr_flows: List[Tensor] = []

    # ------------------------------------------------------------------ helpers
    def _heads(self, convex: bool):
        """The XHeads whose hidden conv runs this forward, flow first: (name, head) pairs."""
        heads = [("flow", self.flow_pred)]
        if convex:
            heads.append(("mask", self.mask_pred))
        if self._with_occlusion:
            heads.append(("occ", self.occlusion_pred))
        return heads

    # ------------------------------------------------------------------ forward
    def forward(self, feat1: Tensor, feat2: Tensor, flow: Tensor, h_feat: Tensor, cxt_feat: Tensor):
        if feat1.device.type != "cuda":
            raise ScflowError(f"{type(self).__name__} runs on the gfx950 HIP kernels only; move "
                              "inputs to a ROCm device (there is no CPU fallback)")
        with torch.no_grad():
            return self._forward(feat1, feat2, flow, h_feat, cxt_feat)

    def _forward(self, feat1, feat2, flow, h_feat, cxt_feat, hx: Optional[Tensor] = None):
        """``hx``: optional channels-last [N·h·w, hx_channels] buffer whose first hc + xc channels
        already hold tanh(h) | relu(cxt) (the refiners write the context encoder's output there
        directly); h_feat / cxt_feat are then ignored."""
        dev = feat1.device
        f32 = torch.float32
        feat1 = feat1.contiguous().float()
        feat2 = feat2.contiguous().float()
        N, _, h, w = feat1.shape
        scale = 2 ** (self.num_levels - 1)
        H, W = scale * h, scale * w
        M = N * h * w
        iters = int(self.iters)
        if tuple(flow.shape) != (N, 2, h, w):
            raise ValueError(f"flow must be [{N}, 2, {h}, {w}] (the feature resolution), got "
                             f"{tuple(flow.shape)}")
        convex = bool(self.convex_upsample_flow)
        if convex and (scale != 8 or 2 * self.radius + 1 != 9):
            raise NotImplementedError("convex upsampling: scale 8 (num_levels 4) and a 3×3 "
                                      "neighbourhood (radius 4) only")

        # the pyramid, the channels-last working set and the iteration up to the GRU: the shared
        # core (recurrent.py), everything on the current stream
        core = RecurrentCore(self, feat1, feat2)
        core.bind_state(h_feat, cxt_feat, hx)
        hx_flow, hid = core.hx_flow, core.hid
        # the low-resolution flow, double-buffered: iteration i reads F2s[i % 2] (lookup, flow
        # branch, the tail's neighbourhoods) and its tail writes F2s[(i + 1) % 2]
        F2s = [torch.empty(M, 2, device=dev, dtype=f32) for _ in range(2)]
        flow = flow.contiguous().float()
        ops.nchw_into(flow, Chan.whole(F2s[0]))
        ops.nchw_into(flow, hx_flow)
        heads = self._heads(convex)
        widths = [hd.layers[-1].conv.out_channels for _, hd in heads]
        offs = {nm: (sum(widths[:i]), widths[i]) for i, (nm, _) in enumerate(heads)}
        HEAD = torch.empty(M, sum(widths), device=dev, dtype=f32)
        D2 = torch.empty(M, 2, device=dev, dtype=f32)
        LOGITS = torch.empty(M, self.mask_channels, device=dev, dtype=f32) if convex else None
        OCC = torch.empty(M, 1, device=dev, dtype=f32) if self._with_occlusion else None

        # outputs (stacked; the lists returned are views)
        o_flow = torch.empty(iters, N, 2, H, W, device=dev, dtype=f32)
        o_occ = torch.empty(iters, N, 1, H, W, device=dev, dtype=f32) if self._with_occlusion \
            else None

        head_runner = self._hidden_heads(heads)
        flow_pred_r = ConvRunner.of(self.flow_pred.predict_layer, None)
        mask_pred_r = ConvRunner.of(self.mask_pred.predict_layer, None)
        occ_pred_r = ConvRunner.of(self.occlusion_pred.predict_layer, "Sigmoid") \
            if self._with_occlusion else None

        def seg_heads():  # hidden convs (one launch where the heads allow), then the predictors
            if head_runner is not None:
                head_runner.run(hid, Chan.whole(HEAD), N, h, w)
            else:
                for nm, hd in heads:
                    run_chain(hd.layers, hid, Chan(HEAD, *offs[nm]), N, h, w)
            flow_pred_r.run(Chan(HEAD, *offs["flow"]), Chan.whole(D2), N, h, w)
            if convex:
                mask_pred_r.run(Chan(HEAD, *offs["mask"]), Chan.whole(LOGITS), N, h, w)
            if occ_pred_r is not None:
                occ_pred_r.run(Chan(HEAD, *offs["occ"]), Chan.whole(OCC), N, h, w)

        # the tail's launches take per-iteration output pointers: their argument lists are built
        # once for every iteration and replayed like the recorded segments
        tails = []
        for j in range(iters):
            calls = []
            cur, nxt = F2s[j % 2], Chan.whole(F2s[(j + 1) % 2])
            with ops.binding(calls, run=False):
                if convex:
                    ops.convex_upsample(Chan.whole(LOGITS), cur, D2, OCC, N, h, w, o_flow[j],
                                        None if o_occ is None else o_occ[j], next0=nxt,
                                        next1=hx_flow, logit_scale=0.25, value_scale=float(scale),
                                        scale=scale)
                else:  # the reference's `mask is None` branch: bilinear, the occlusion unscaled
                    ops.flow_upsample(cur, D2, OCC, N, h, w, H, W, float(scale), o_flow[j],
                                      None if o_occ is None else o_occ[j])
                    ops.flow_add(cur, D2, nxt, N, h, w, out1=hx_flow)
            tails.append(calls)
        if self.keep_lr_flows:
            self.lr_flows = []
        # last_plan's keys (hoist: hoisted context)
        self._last_plan = dict(convex=convex, fuse_lc=core.fuse_lc, tiled=core.tiled,
                               hoist=core.ctx_map is not None)
        if core.gru_bf16:
            self._last_plan["gru_bf16"] = True
        if core.menc_bf16:
            self._last_plan["menc_bf16"] = True

        for it in range(iters):
            par = str(it % 2)
            F2 = F2s[it % 2]
            core.flow_branch(par, F2)
            core.correlation(par, F2)
            core.motion_out()
            core.gru()
            core.segment("heads", seg_heads)
            for c in tails[it]:
                c()
            if self.keep_lr_flows:
                self.lr_flows.append(ops.chan_to_nchw(Chan.whole(F2s[(it + 1) % 2]), N, h, w))
        return self._result(o_flow, o_occ)

    def _result(self, o_flow: Tensor, o_occ: Optional[Tensor]):
        return list(o_flow.unbind(0))


@MODELS.register_module()
class RAFTDecoderMask(RAFTDecoder):
    """raft_decoder_mask.py:21-208: RAFTDecoder plus the occlusion head (1×1 predictor, sigmoid),
    upsampled with the flow's weights; returns (upflow_preds, upocclusion_preds)."""
    _with_occlusion = True

    def _result(self, o_flow: Tensor, o_occ: Optional[Tensor]):
        return list(o_flow.unbind(0)), list(o_occ.unbind(0))
