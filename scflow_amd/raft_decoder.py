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
* ``iters`` times: lookup (fused with corr_net.0 where SCFlowDecoder fuses it) → motion encoder →
  GRU → the hidden convs of the two or three XHeads as ONE launch (cout 512 / 768) → the 3×3 flow
  predictor, the 1×1 mask predictor (576 logits) and the 1×1 occlusion predictor with its sigmoid
  → ``scflow_convex_upsample``: one softmax per sub-pixel serves the ×8 flow and the ×8 occlusion,
  and the same launch writes flow + Δflow into the next iteration's lookup buffer and into HX's
  flow channels.  The low-resolution flow alternates between two buffers (the launch reads its
  neighbours' pixels, so it cannot update the flow in place).

The launches whose arguments do not change between iterations are recorded once (``ops.binding``)
and replayed; no host synchronisation happens inside ``forward``.  There is no CPU path, no second
stream and no deferred full-resolution work here.  ``net_type='Small'`` is not supported.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import ScflowError
from .modules import (ConvGRU, ConvRunner, CorrelationPyramid, CorrLookup, MotionEncoder, XHead,
                      run_chain)
from .ops import Chan
from .registry import MODELS

Tensor = torch.Tensor


@MODELS.register_module()
class RAFTDecoder(nn.Module):
    _h_channels = {"Basic": 128, "Small": 96}
    _cxt_channels = {"Basic": 128, "Small": 64}
    _with_occlusion = False

    def __init__(self, net_type: str, num_levels: int, radius: int, iters: int,
                 corr_lookup_cfg: dict = dict(type="CorrLookup", align_corners=True),
                 gru_type: str = "SeqConv", feat_channels: Union[int, Sequence[int]] = 256,
                 mask_channels: int = 64, convex_unsample_flow: bool = True,
                 conv_cfg: Optional[dict] = None, norm_cfg: Optional[dict] = None,
                 act_cfg: Optional[dict] = None) -> None:
        super().__init__()
        assert net_type in ["Basic", "Small"]
        assert type(feat_channels) in (int, tuple, list)
        if net_type == "Small":
            raise NotImplementedError("net_type Small (82 / 96 / 64-channel tensors, no mask "
                                      "predictor) is not supported by the HIP RAFT decoders")
        self.corr_block = CorrelationPyramid(num_levels=num_levels)
        feat_channels = list(feat_channels) if isinstance(feat_channels, (tuple, list)) \
            else [feat_channels]
        self.net_type = net_type
        self.num_levels = num_levels
        self.radius = radius
        self.h_channels = self._h_channels.get(net_type)
        self.cxt_channels = self._cxt_channels.get(net_type)
        self.iters = iters
        # raft_decoder.py:356: the 3×3 neighbourhood's 9 taps are spelt 2·radius + 1
        self.mask_channels = mask_channels * (2 * radius + 1)
        corr_lookup_cfg = dict(corr_lookup_cfg)
        corr_lookup_cfg.pop("type", None)
        corr_lookup_cfg["radius"] = radius
        self.corr_lookup = CorrLookup(**corr_lookup_cfg)
        self.encoder = MotionEncoder(num_levels=num_levels, radius=radius, net_type=net_type,
                                     conv_cfg=conv_cfg, norm_cfg=norm_cfg, act_cfg=act_cfg)
        self.gru_type = gru_type
        self.gru = self.make_gru_block()
        self.flow_pred = XHead(self.h_channels, feat_channels, 2, x="flow")
        if self._with_occlusion:
            self.occlusion_pred = XHead(self.h_channels, feat_channels, 1, x="mask")
        self.mask_pred = XHead(self.h_channels, feat_channels, self.mask_channels, x="mask")
        self.convex_upsample_flow = convex_unsample_flow
        self._head_runners = {}
        # compute the context features' (loop-invariant) GRU contribution once per forward
        self.hoist_context = True
        # SCFlowDecoder's attributes and thresholds (measured there): the pyramid in the tiled
        # layout when the geometry allows it; the lookup and corr_net.0 as one launch on feature
        # maps of at most 32 × 32.  Off: the paths larger or untileable maps take (the tests run
        # them at 32 × 32 this way)
        self.tiled_pyramid = True
        self.fuse_lookup_conv = True
        self.fuse_lookup_conv_max_px = 32 * 32
        # also keep the low-resolution flow after every iteration (flow + Δflow, NCHW) in
        # ``lr_flows``: one transpose launch per iteration; for tests and warm starts
        self.keep_lr_flows = False
        self.lr_flows: List[Tensor] = []

    def make_gru_block(self):
        return ConvGRU(self.h_channels, self.encoder.out_channels[0] + 2 + self.cxt_channels,
                       net_type=self.gru_type)

    # ------------------------------------------------------------------ helpers
    @property
    def hx_channels(self) -> int:
        """Channels of the channels-last GRU working buffer: [h | cxt | motion | flow]."""
        return self.h_channels + self.cxt_channels + self.encoder.out_channels[0] + 2

    @property
    def last_plan(self) -> Optional[dict]:
        """The schedule the last forward took (read-only copy; None before the first): the
        booleans ``convex``, ``fuse_lc`` (fused lookup + 1×1), ``tiled`` (tiled pyramid) and
        ``hoist`` (hoisted context)."""
        plan = getattr(self, "_last_plan", None)
        return None if plan is None else dict(plan)

    def _heads(self, convex: bool):
        """The XHeads whose hidden conv runs this forward, flow first: (name, head) pairs."""
        heads = [("flow", self.flow_pred)]
        if convex:
            heads.append(("mask", self.mask_pred))
        if self._with_occlusion:
            heads.append(("occ", self.occlusion_pred))
        return heads

    def _hidden_heads(self, heads) -> Optional[ConvRunner]:
        """The heads' first hidden convs as one launch when they have one layer of one shape."""
        layers = [hd.layers for _, hd in heads]
        c0 = layers[0][0].conv
        if any(len(ls) != 1 or ls[0].conv.kernel_size != c0.kernel_size or
               ls[0].conv.padding != c0.padding for ls in layers):
            return None
        key = tuple(nm for nm, _ in heads)
        if key not in self._head_runners:
            self._head_runners[key] = ConvRunner([ls[0].conv for ls in layers], "ReLU")
        return self._head_runners[key]

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
        hc, xc = self.h_channels, self.cxt_channels
        co = self.encoder.out_channels[0]
        hx_c = self.hx_channels
        iters = int(self.iters)
        if tuple(flow.shape) != (N, 2, h, w):
            raise ValueError(f"flow must be [{N}, 2, {h}, {w}] (the feature resolution), got "
                             f"{tuple(flow.shape)}")
        convex = bool(self.convex_upsample_flow)
        if convex and (scale != 8 or 2 * self.radius + 1 != 9):
            raise NotImplementedError("convex upsampling: scale 8 (num_levels 4) and a 3×3 "
                                      "neighbourhood (radius 4) only")

        # correlation pyramid (once per forward)
        tiled = self.tiled_pyramid and ops.tiled_lookup_ok(h, w, self.num_levels, self.radius,
                                                           self.corr_lookup.align_corners)
        if tiled:
            pyr = ops.corr_pyramid_tiled(feat1, feat2, self.num_levels)
        else:
            pyr, _ = ops.corr_pyramid(feat1, feat2, self.num_levels)

        # channels-last working set
        if hx is not None:
            if hx.shape != (M, hx_c) or hx.dtype != f32 or not hx.is_contiguous():
                raise ValueError(f"hx must be a contiguous float32 [{M}, {hx_c}] buffer")
            HX = hx
        else:
            HX = torch.empty(M, hx_c, device=dev, dtype=f32)
            ops.nchw_into(h_feat.contiguous().float(), Chan(HX, 0, hc))
            ops.nchw_into(cxt_feat.contiguous().float(), Chan(HX, hc, xc))
        ctx_map = self.gru.context_map(Chan(HX, hc, xc), N, h, w) if self.hoist_context else None
        hx_flow = Chan(HX, hx_c - 2, 2)
        hx_motion = Chan(HX, hc + xc, co)
        hid = Chan(HX, 0, hc)
        # the low-resolution flow, double-buffered: iteration i reads F2s[i % 2] (lookup, flow
        # branch, the tail's neighbourhoods) and its tail writes F2s[(i + 1) % 2]
        F2s = [torch.empty(M, 2, device=dev, dtype=f32) for _ in range(2)]
        flow = flow.contiguous().float()
        ops.nchw_into(flow, Chan.whole(F2s[0]))
        ops.nchw_into(flow, hx_flow)
        K_look = self.num_levels * (2 * self.radius + 1) ** 2
        CORR = torch.empty(M, K_look, device=dev, dtype=f32)
        cc = self.encoder.corr_net[-1].conv.out_channels
        cf = self.encoder.flow_net[-1].conv.out_channels
        MF = torch.empty(M, cc + cf, device=dev, dtype=f32)
        Z = torch.empty(M, hc, device=dev, dtype=f32)
        RH = torch.empty(M, hc, device=dev, dtype=f32)
        heads = self._heads(convex)
        widths = [hd.layers[-1].conv.out_channels for _, hd in heads]
        offs = {nm: (sum(widths[:i]), widths[i]) for i, (nm, _) in enumerate(heads)}
        HEAD = torch.empty(M, sum(widths), device=dev, dtype=f32)
        D2 = torch.empty(M, 2, device=dev, dtype=f32)
        LOGITS = torch.empty(M, self.mask_channels, device=dev, dtype=f32) if convex else None
        OCC = torch.empty(M, 1, device=dev, dtype=f32) if self._with_occlusion else None

        def scratch(mods):
            return [torch.empty(M, m.conv.out_channels, device=dev, dtype=f32) for m in mods[:-1]]

        s_corr = scratch(self.encoder.corr_net)
        s_flow = scratch(self.encoder.flow_net)
        s_out = scratch(self.encoder.out_net)

        # outputs (stacked; the lists returned are views)
        o_flow = torch.empty(iters, N, 2, H, W, device=dev, dtype=f32)
        o_occ = torch.empty(iters, N, 1, H, W, device=dev, dtype=f32) if self._with_occlusion \
            else None

        head_runner = self._hidden_heads(heads)
        flow_pred_r = ConvRunner.of(self.flow_pred.predict_layer, None)
        mask_pred_r = ConvRunner.of(self.mask_pred.predict_layer, None)
        occ_pred_r = ConvRunner.of(self.occlusion_pred.predict_layer, "Sigmoid") \
            if self._with_occlusion else None

        # the launches that read and write the same persistent buffers in every iteration are
        # recorded on their first pass and replayed afterwards (one ctypes call each); the ones
        # that read the flow are recorded once per parity of the double buffer
        rec = {}

        def segment(name, fn):
            calls = rec.get(name)
            if calls is None:
                calls = rec[name] = []
                with ops.binding(calls):
                    fn()
            else:
                for c in calls:
                    c()

        gru_step = self.gru.bind_step(Chan.whole(HX), Chan.whole(Z), Chan.whole(RH), N, h, w,
                                      ctx_map=ctx_map, cxt_channels=xc)
        F2 = F2s[0]

        def seg_flow_branch():
            run_chain(self.encoder.flow_net, Chan.whole(F2), Chan(MF, cc, cf), N, h, w, s_flow)

        def seg_lookup():
            ops.corr_lookup(pyr, F2, N, h, w, self.num_levels, self.radius, out=Chan.whole(CORR),
                            flow_layout="nhwc", align_corners=self.corr_lookup.align_corners,
                            tiled=tiled)

        corr_net = self.encoder.corr_net
        c0m = corr_net[0].conv
        fuse_lc = (self.fuse_lookup_conv and h * w <= self.fuse_lookup_conv_max_px and tiled and
                   len(corr_net) == 2 and
                   tuple(c0m.kernel_size) == (1, 1) and tuple(c0m.stride) == (1, 1) and
                   tuple(c0m.padding) == (0, 0) and
                   ops.lookup_conv1x1_ok(h, w, self.num_levels, self.radius, c0m.in_channels,
                                         c0m.out_channels))

        def seg_lookup_conv():  # lookup + corr_net.0 in one launch
            r0 = ConvRunner.of(c0m, corr_net[0].act_type)
            packed, bias = r0.packed(c0m.in_channels, 0, w, _lib.CONV_1X1W)
            ops.corr_lookup_conv1x1(pyr, F2, packed, bias, Chan.whole(s_corr[-1]), N, h, w,
                                    self.num_levels, self.radius, c0m.out_channels,
                                    corr_net[0].act_type, self.corr_lookup.align_corners)

        def seg_corr_hidden():  # corr_net.0 (1×1 324→256)
            if len(corr_net) > 1:
                run_chain(corr_net[:-1], Chan.whole(CORR), Chan.whole(s_corr[-1]), N, h, w,
                          s_corr[:-1])

        def seg_corr_last():  # corr_net.1 (3×3 256→192)
            src = Chan.whole(s_corr[-1]) if len(corr_net) > 1 else Chan.whole(CORR)
            ConvRunner.of(corr_net[-1].conv, corr_net[-1].act_type).run(src, Chan(MF, 0, cc), N, h, w)

        def seg_out():
            run_chain(self.encoder.out_net, Chan.whole(MF), hx_motion, N, h, w, s_out)

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
        self._last_plan = dict(convex=convex, fuse_lc=bool(fuse_lc), tiled=bool(tiled),
                               hoist=ctx_map is not None)

        for it in range(iters):
            par = str(it % 2)
            F2 = F2s[it % 2]
            segment("flow_branch" + par, seg_flow_branch)
            if fuse_lc:
                segment("lookup_conv" + par, seg_lookup_conv)
            else:
                segment("lookup" + par, seg_lookup)
                segment("corr_hidden", seg_corr_hidden)
            segment("corr_last", seg_corr_last)
            segment("out", seg_out)
            gru_step()
            segment("heads", seg_heads)
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
