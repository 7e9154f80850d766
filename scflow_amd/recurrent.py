"""The recurrent core SCFlowDecoder and the RAFT decoders share: the decoder base class (the
submodules up to the GRU and the knobs that plan them), the planning of the tiled pyramid and the
fused lookup + corr_net.0, and ``RecurrentCore`` — one forward's correlation pyramid, channels-last
working set ``HX = [h | cxt | motion | flow]``, recorded launch segments and the iteration's steps
up to the GRU (flow branch, correlation branch, out_net, GRU).

Everything after the GRU is the decoder's own: ``decoder.py`` keeps the heads' predictors, the
Δflow / mask encoders, the pose head, the fused tail with its deferred full-resolution work, the
streams, events and kernel-timer hooks; ``raft_decoder.py`` keeps the head predictors and the
convex / bilinear upsampling tail.  The core launches on whatever stream is current when a step is
called and knows nothing of either tail.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn

from . import _lib, ops
from .modules import (ConvGRU, ConvRunner, CorrelationPyramid, CorrLookup, MotionEncoder,
                      run_chain)
from .ops import Chan

Tensor = torch.Tensor


def plan_correlation(tiled_pyramid: bool, fuse_lookup_conv: bool, fuse_lookup_conv_max_px: int,
                     corr_net, h: int, w: int, num_levels: int, radius: int,
                     align_corners: bool) -> Tuple[bool, bool]:
    """(tiled, fuse_lc) for an h×w feature map: whether the pyramid takes the tiled layout, and
    whether the lookup and corr_net.0 (a 1×1 conv) run as one launch.  Reads the decoder's knobs
    and ``corr_net``'s shapes only; touches no tensor."""
    tiled = bool(tiled_pyramid and ops.tiled_lookup_ok(h, w, num_levels, radius, align_corners))
    c0 = corr_net[0].conv
    fuse_lc = bool(fuse_lookup_conv and h * w <= fuse_lookup_conv_max_px and tiled and
                   len(corr_net) == 2 and
                   tuple(c0.kernel_size) == (1, 1) and tuple(c0.stride) == (1, 1) and
                   tuple(c0.padding) == (0, 0) and
                   ops.lookup_conv1x1_ok(h, w, num_levels, radius, c0.in_channels, c0.out_channels))
    return tiled, fuse_lc


class _RecurrentDecoder(nn.Module):
    """What the decoders' constructors share: corr_block, corr_lookup, encoder and gru (registered
    in this order, before the subclass's heads), the channel tables and the knobs of the core."""
    _h_channels = {"Basic": 128, "Small": 96}
    _cxt_channels = {"Basic": 128, "Small": 64}

    def __init__(self, net_type: str, num_levels: int, radius: int, iters: int,
                 corr_lookup_cfg: dict, gru_type: str, feat_channels: Union[int, Sequence[int]],
                 conv_cfg: Optional[dict], norm_cfg: Optional[dict],
                 act_cfg: Optional[dict]) -> None:
        super().__init__()
        assert net_type in ["Basic", "Small"]
        assert type(feat_channels) in (int, tuple, list)
        self.corr_block = CorrelationPyramid(num_levels=num_levels)
        self.feat_channels = list(feat_channels) if isinstance(feat_channels, (tuple, list)) \
            else [feat_channels]
        self.net_type = net_type
        self.num_levels = num_levels
        self.radius = radius
        self.h_channels = self._h_channels.get(net_type)
        self.cxt_channels = self._cxt_channels.get(net_type)
        self.iters = iters
        corr_lookup_cfg = dict(corr_lookup_cfg)
        corr_lookup_cfg.pop("type", None)  # the RAFT configs' default carries one
        corr_lookup_cfg["radius"] = radius
        self.corr_lookup = CorrLookup(**corr_lookup_cfg)
        self.encoder = MotionEncoder(num_levels=num_levels, radius=radius, net_type=net_type,
                                     conv_cfg=conv_cfg, norm_cfg=norm_cfg, act_cfg=act_cfg)
        self.gru_type = gru_type
        self.gru = self.make_gru_block()
        self._head_runners = {}
        # compute the context features' (loop-invariant) GRU contribution once per forward
        self.hoist_context = True
        # correlation pyramid in the tiled layout (4×4 tiles of 16 floats per map, pooling fused
        # into the GEMM epilogue; ops.corr_pyramid_tiled) when the geometry allows it
        self.tiled_pyramid = True
        # the lookup and corr_net.0 (1×1 324→256) as ONE launch (scflow_corr_lookup_conv1x1: the
        # correlation features stay in LDS) when the geometry allows (tiled pyramid, L = 4, r = 4)
        # and the feature map has at most 32×32 pixels: measured on SCFlowDecoder, 5.112 vs 5.131
        # ms/forward at configs[1] (round 5, tools/sess_r5d.sh), but 49.2 vs 48.0 ms at configs[4]
        # (64×64), where the separate lookup (tile-row regions) and 1×1 conv win.  Off: the paths
        # larger or untileable maps take (the tests run them at 32 × 32 this way)
        self.fuse_lookup_conv = True
        self.fuse_lookup_conv_max_px = 32 * 32
        # the GRU's z|r and q convs on the bf16 direct kernel (ConvGRU.bf16): operands rounded to
        # bf16, fp32 accumulation, every buffer fp32.  Inference only, off by default, read at
        # every forward; a feature map the kernel does not cover raises ScflowError (no fallback).
        # last_plan carries gru_bf16=True only for a forward that ran it.
        self.gru_bf16 = False
        # the motion encoder's 3×3 convs (corr_net's last, flow_net's last, out_net) on the bf16
        # direct 3×3 kernel (MotionEncoder.bf16), under the same terms: operands rounded to bf16,
        # fp32 accumulation and buffers, inference only, off by default, read at every forward,
        # ScflowError on an uncovered feature map, last_plan carries menc_bf16=True only for a
        # forward that ran it.  Independent of gru_bf16.
        self.menc_bf16 = False

    def make_gru_block(self):
        return ConvGRU(self.h_channels, self.encoder.out_channels[0] + 2 + self.cxt_channels,
                       net_type=self.gru_type)

    @property
    def hx_channels(self) -> int:
        """Channels of the channels-last GRU working buffer: [h | cxt | motion | flow]."""
        return self.h_channels + self.cxt_channels + self.encoder.out_channels[0] + 2

    @property
    def last_plan(self) -> Optional[dict]:
        """The schedule the last forward took (read-only copy; None before the first): booleans,
        ``fuse_lc`` (fused lookup + 1×1) and ``tiled`` (tiled pyramid) among them; each decoder
        names its keys where it stores them."""
        plan = getattr(self, "_last_plan", None)
        return None if plan is None else dict(plan)

    def plan_correlation(self, h: int, w: int) -> Tuple[bool, bool]:
        """``plan_correlation`` with this decoder's knobs and geometry: (tiled, fuse_lc)."""
        return plan_correlation(self.tiled_pyramid, self.fuse_lookup_conv,
                                self.fuse_lookup_conv_max_px, self.encoder.corr_net, h, w,
                                self.num_levels, self.radius, self.corr_lookup.align_corners)

    def _hidden_heads(self, heads) -> Optional[ConvRunner]:
        """The (name, XHead) pairs' first hidden convs as one launch when every head has one
        layer of one shape; None otherwise."""
        layers = [hd.layers for _, hd in heads]
        c0 = layers[0][0].conv
        if any(len(ls) != 1 or ls[0].conv.kernel_size != c0.kernel_size or
               ls[0].conv.padding != c0.padding for ls in layers):
            return None
        key = tuple(nm for nm, _ in heads)
        if key not in self._head_runners:
            self._head_runners[key] = ConvRunner([ls[0].conv for ls in layers], "ReLU")
        return self._head_runners[key]


def _no_hook(name: str, start: bool) -> None:
    return None


def _no_hooks_for(*names):
    return None


class RecurrentCore:
    """One forward's shared state, built by either decoder on the stream its forward runs on.

    ``RecurrentCore(...)`` plans the correlation and launches the pyramid; ``bind_state`` then
    fills (or adopts) ``HX``, hoists the context, allocates the motion encoder's buffers and binds
    the GRU step.  (Two calls, because SCFlowDecoder lifts its points between them.)  Per
    iteration the decoder calls ``flow_branch``, ``correlation``, ``motion_out`` and ``gru``, with
    its own forks, joins and deferred work in between.

    ``hook(name, start)`` brackets a launch with a kernel timer and ``hooks_for(*names)`` gives
    ``run_chain`` its per-layer timers; both default to none.  ``segment`` records a group of
    launches on its first pass (``ops.binding``: argument structs built once) and replays them as
    one ctypes call each afterwards, so a name stands for one set of buffers: the steps that read
    the double-buffered flow take the iteration's parity suffix ``par``."""

    def __init__(self, dec: _RecurrentDecoder, feat1: Tensor, feat2: Tensor, hook=None,
                 hooks_for=None) -> None:
        self.dec = dec
        self.hook = hook or _no_hook
        self.hooks_for = hooks_for or _no_hooks_for
        self.dev = feat1.device
        self.N, _, self.h, self.w = feat1.shape
        self.M = self.N * self.h * self.w
        self.tiled, self.fuse_lc = dec.plan_correlation(self.h, self.w)
        self.hook("corr_pyramid", True)
        if self.tiled:
            self.pyr = ops.corr_pyramid_tiled(feat1, feat2, dec.num_levels)
        else:
            self.pyr, _ = ops.corr_pyramid(feat1, feat2, dec.num_levels)
        self.hook("corr_pyramid", False)
        self._rec = {}

    def bind_state(self, h_feat: Optional[Tensor], cxt_feat: Optional[Tensor],
                   hx: Optional[Tensor] = None) -> None:
        """``hx``: a channels-last [M, hx_channels] buffer whose first hc + xc channels already
        hold tanh(h) | relu(cxt); else a fresh one is filled from ``h_feat`` / ``cxt_feat``."""
        dec, N, h, w, M = self.dec, self.N, self.h, self.w, self.M
        dev, f32 = self.dev, torch.float32
        hc, xc = dec.h_channels, dec.cxt_channels
        co = dec.encoder.out_channels[0]
        hx_c = dec.hx_channels
        if hx is not None:
            if hx.shape != (M, hx_c) or hx.dtype != f32 or not hx.is_contiguous():
                raise ValueError(f"hx must be a contiguous float32 [{M}, {hx_c}] buffer")
            HX = hx
        else:
            HX = torch.empty(M, hx_c, device=dev, dtype=f32)
            ops.nchw_into(h_feat.contiguous().float(), Chan(HX, 0, hc))
            ops.nchw_into(cxt_feat.contiguous().float(), Chan(HX, hc, xc))
        self.HX = HX
        self.gru_bf16 = dec.gru.bf16 = bool(dec.gru_bf16)
        self.menc_bf16 = dec.encoder.bf16 = bool(dec.menc_bf16)
        dec.encoder.runners()  # (sets or clears the 3×3 runners' format before they are bound)
        # loop-invariant context share of the GRU pre-activations (once per forward)
        self.ctx_map = dec.gru.context_map(Chan(HX, hc, xc), N, h, w) if dec.hoist_context else None
        self.hx_flow = Chan(HX, hx_c - 2, 2)
        self.hx_motion = Chan(HX, hc + xc, co)
        self.hid = Chan(HX, 0, hc)
        enc = dec.encoder
        self.CORR = torch.empty(M, dec.num_levels * (2 * dec.radius + 1) ** 2, device=dev, dtype=f32)
        self.cc = enc.corr_net[-1].conv.out_channels
        self.cf = enc.flow_net[-1].conv.out_channels
        self.MF = torch.empty(M, self.cc + self.cf, device=dev, dtype=f32)
        # (the bound launches hold addresses, not tensors: every buffer they touch is kept here)
        self.Z = torch.empty(M, hc, device=dev, dtype=f32)
        self.RH = torch.empty(M, hc, device=dev, dtype=f32)
        self.s_corr = self.scratch(enc.corr_net)
        self.s_flow = self.scratch(enc.flow_net)
        self.s_out = self.scratch(enc.out_net)

    def scratch(self, mods):
        """The buffers between a Sequential's ConvModules (every output but the last)."""
        return [torch.empty(self.M, m.conv.out_channels, device=self.dev, dtype=torch.float32)
                for m in mods[:-1]]

    def segment(self, name: str, fn, *args) -> None:
        calls = self._rec.get(name)
        if calls is None:
            calls = self._rec[name] = []
            with ops.binding(calls):
                fn(*args)
        else:
            for c in calls:
                c()

    # ------------------------------------------------------------------ the iteration's steps
    def flow_branch(self, par: str, flow_in: Tensor) -> None:
        """flow_net on ``flow_in`` [M, 2] → the motion features' flow half."""
        self.segment("flow_branch" + par, self._flow_branch, flow_in)

    def correlation(self, par: str, F2: Tensor, mask: Optional[Tensor] = None) -> None:
        """Lookup at the flow ``F2`` [M, 2] (samples scaled by ``mask`` [M] when given) and
        corr_net → the motion features' correlation half: the lookup and corr_net.0 as one launch
        where planned, else the lookup, then corr_net's hidden convs; then corr_net's last conv."""
        hook, segment = self.hook, self.segment
        if self.fuse_lc:
            hook("corr_lookup_conv", True)
            segment("lookup_conv" + par, self._lookup_conv, F2, mask)
            hook("corr_lookup_conv", False)
        else:
            hook("corr_lookup", True)
            segment("lookup" + par, self._lookup, F2, mask)
            hook("corr_lookup", False)
            segment("corr_hidden", self._corr_hidden)
        hook("corr_net1", True)
        segment("corr_last", self._corr_last)
        hook("corr_net1", False)

    def motion_out(self) -> None:
        """out_net on [corr | flow] features → HX's motion channels."""
        self.segment("out", self._out)

    def gru(self, hooks=None) -> None:
        """The GRU step, in place on HX's hidden channels (``hooks``: ConvGRU.step's, read on
        the recording pass)."""
        self.segment("gru", self._gru, hooks)

    # ------------------------------------------------------------------ the recorded launches
    def _gru(self, hooks):
        dec = self.dec
        dec.gru.step(Chan.whole(self.HX), Chan.whole(self.Z), Chan.whole(self.RH), self.N, self.h,
                     self.w, hooks=hooks, ctx_map=self.ctx_map, cxt_channels=dec.cxt_channels)

    def _flow_branch(self, flow_in):
        run_chain(self.dec.encoder.flow_net, Chan.whole(flow_in), Chan(self.MF, self.cc, self.cf),
                  self.N, self.h, self.w, self.s_flow, hooks=self.hooks_for(None, "flow_net1"))

    def _lookup(self, F2, mask):
        dec = self.dec
        ops.corr_lookup(self.pyr, F2, self.N, self.h, self.w, dec.num_levels, dec.radius,
                        out=Chan.whole(self.CORR), flow_layout="nhwc",
                        align_corners=dec.corr_lookup.align_corners, tiled=self.tiled, mask=mask)

    def _lookup_conv(self, F2, mask):  # lookup + corr_net.0 in one launch
        dec = self.dec
        m0 = dec.encoder.corr_net[0]
        c0 = m0.conv
        packed, bias = ConvRunner.of(c0, m0.act_type).packed(c0.in_channels, 0, self.w,
                                                             _lib.CONV_1X1W)
        ops.corr_lookup_conv1x1(self.pyr, F2, packed, bias, Chan.whole(self.s_corr[-1]), self.N,
                                self.h, self.w, dec.num_levels, dec.radius, c0.out_channels,
                                m0.act_type, dec.corr_lookup.align_corners, mask=mask)

    def _corr_hidden(self):  # corr_net.0 (1×1 324→256)
        corr_net = self.dec.encoder.corr_net
        if len(corr_net) > 1:
            run_chain(corr_net[:-1], Chan.whole(self.CORR), Chan.whole(self.s_corr[-1]), self.N,
                      self.h, self.w, self.s_corr[:-1])

    def _corr_last(self):  # corr_net.1 (3×3 256→192), bracketed by the "corr_net1" hook
        last = self.dec.encoder.corr_net[-1]
        src = Chan.whole(self.s_corr[-1]) if self.s_corr else Chan.whole(self.CORR)
        ConvRunner.of(last.conv, last.act_type).run(src, Chan(self.MF, 0, self.cc), self.N, self.h,
                                                    self.w)

    def _out(self):
        run_chain(self.dec.encoder.out_net, Chan.whole(self.MF), self.hx_motion, self.N, self.h,
                  self.w, self.s_out, hooks=self.hooks_for("out_net"))
