"""SCFlowDecoder — drop-in replacement for the reference decoder, running on gfx950 HIP kernels.

Reference: ``models/decoder/scflow_decoder.py:19-252``.  Same constructor kwargs (:48-68), same
submodules and state-dict keys (so reference checkpoints load), same ``forward`` signature
(:151-156) and the same 7-list return (:252).  ``iters`` is re-read on every call (the refiner
overwrites it temporarily, ``scflow_refiner.py:150-158``).

A forward (B pairs, features h×w = image/8, M = B·h·w) is one ``_DecoderRun``: its constructor
launches what happens once — the correlation pyramid (a1), the dense object-frame points (a9, no
``nonzero``, no host sync), the channels-last working set ``HX = [h | cxt | motion | flow]`` — and
plans the schedule; then, ``iters`` times, two phases:

* ``heavy(it)``: the ↓8 flow (a11↓, first iteration only under the fused tail), the flow branch on
  the side stream beside lookup + corr_net (a2, a3), out_net, the GRU (a4) and the heads' hidden
  convs with their predictors (a5) — the convolutions that fill the chip; the previous iteration's
  deferred full-resolution outputs are queued on the side stream behind the join;
* ``tail(it)``: flow predictor + Δflow encoder ‖ mask predictor + mask encoder (a5, a6; paired
  launches, or two streams), the pose head's trunk (a7, HIP) and the fused pose step (a8 + a10 +
  a11↑ + the next iteration's a11↓; its rotation / translation heads inside the same launch).

No host synchronisation happens inside ``forward``; the whole call can be captured into a
HIP graph (``graph.py``).  There is no CPU path: inputs must be on a ROCm device.

The constructor's common part and the iteration up to the GRU (pyramid, ``HX``, a2–a4, the
recorded segments, the tiled / fused-lookup planning) live in ``recurrent.py``, shared with the
RAFT decoders; this file holds what follows the GRU (a5–a11), the streams and events
(``_Streams``), ping-pong and the kernel-timer hooks.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence, Union

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import ScflowError
from .derived import derived
from .modules import ConvModule, ConvRunner, XHead, run_chain, run_chain_pair
from .ops import Chan
from .recurrent import RecurrentCore, _RecurrentDecoder
from .registry import MODELS

Tensor = torch.Tensor


def _record_on(out, stream) -> None:
    """The forward ran on the decoder's priority stream, so the caching allocator ties its
    outputs' blocks to that stream: record the caller's stream on each one (once per storage)
    so a caller reading them there cannot see the blocks reused before its reads finish."""
    seen = set()
    for item in out:
        for t in (item if isinstance(item, (list, tuple)) else (item,)):
            if isinstance(t, Tensor):
                key = t.untyped_storage().data_ptr()
                if key not in seen:
                    seen.add(key)
                    t.record_stream(stream)


def _alloc_outputs(iters: int, N: int, H: int, W: int, rot_channels: int, dev) -> Dict[str, Tensor]:
    """The seven stacked output tensors of a forward (the lists returned are views)."""
    def e(*shape):
        return torch.empty(iters, N, *shape, device=dev, dtype=torch.float32)
    return dict(flow_pose=e(2, H, W), flow_pred=e(2, H, W), mask=e(1, H, W), R=e(3, 3), t=e(3),
                drot=e(rot_channels), dt=e(3))


def _lists(outs: Dict[str, Tensor]):
    """The reference's 7-list return: per-iteration views of the stacked outputs."""
    return tuple(list(outs[k].unbind(0))
                 for k in ("flow_pose", "flow_pred", "R", "t", "mask", "drot", "dt"))


def _at(bufs, i: int) -> Tensor:
    """Buffer ``i`` of a list that holds two buffers where the plan double-buffers them (indexed
    by parity) and one where it does not."""
    return bufs[i % len(bufs)]


class _Streams:
    """A forward's (main, side) streams, their raw handles and the orderings the forward uses.

    ``events`` = (fork, join, mark), each with ``record(s)`` / ``wait(s)``: ``ops.SyncEvent``
    (device scope: no system-scope cache writeback per record) on the raw handles (``raw``), or
    ``torch.cuda.Event`` on the stream objects.  They are reused every iteration (a wait captures
    the event's state when issued).  Without events, or with ``side is main``, everything runs on
    the main stream and every method is a no-op."""

    def __init__(self, main, side, events=None, raw: bool = True) -> None:
        self.main, self.side = main, (main if events is None else side)
        self.h_main, self.h_side = main.cuda_stream, self.side.cuda_stream
        self.two = self.side is not main
        self._m, self._s = (self.h_main, self.h_side) if raw else (main, self.side)
        self._fork, self._join, self._mark = events if self.two else (None, None, None)

    @classmethod
    def of(cls, dec: "SCFlowDecoder", dev, slot=0) -> "_Streams":
        """The current stream + ``dec``'s side stream of this slot, with ``dec``'s event flavour."""
        main = torch.cuda.current_stream(dev)
        if not dec.side_stream:
            return cls(main, main)
        side = dec._side_stream(dev, slot)
        if dec.device_scope_events:
            evs = dec._sync_events(dev, slot) + dec._sync_events(dev, (slot, "full"))[:1]
            return cls(main, side, evs)
        return cls(main, side, tuple(torch.cuda.Event() for _ in range(3)), raw=False)

    def fork(self) -> None:
        """The side stream waits for what the main stream holds now."""
        if self.two:
            self._fork.record(self._m)
            self._fork.wait(self._s)

    def join(self) -> None:
        """The main stream waits for what the side stream holds now."""
        if self.two:
            self._join.record(self._s)
            self._join.wait(self._m)

    def mark_side(self) -> None:
        """Mark the side stream's position (after a deferred launch) …"""
        if self.two:
            self._mark.record(self._s)

    def wait_side_mark(self) -> None:
        """… and have the main stream wait for the last mark (see ``_DecoderRun.tail``)."""
        if self.two:
            self._mark.wait(self._m)


@MODELS.register_module()
class SCFlowDecoder(_RecurrentDecoder):
    def __init__(self, net_type: str, num_levels: int, radius: int, iters: int, detach_flow: bool,
                 detach_mask: bool, detach_pose: bool, mask_flow: bool, mask_corr: bool,
                 pose_head_cfg: dict, depth_transform: str = "exp", detach_depth_for_xy: bool = False,
                 corr_lookup_cfg: dict = dict(align_corners=True), gru_type: str = "SeqConv",
                 feat_channels: Union[int, Sequence[int]] = 256, conv_cfg: Optional[dict] = None,
                 norm_cfg: Optional[dict] = None, act_cfg: Optional[dict] = None) -> None:
        super().__init__(net_type, num_levels, radius, iters, corr_lookup_cfg, gru_type,
                         feat_channels, conv_cfg, norm_cfg, act_cfg)
        self.detach_flow = detach_flow
        self.detach_mask = detach_mask
        self.detach_pose = detach_pose
        self.detach_depth_for_xy = detach_depth_for_xy
        self.mask_flow = mask_flow
        self.mask_corr = mask_corr
        self.depth_transform = depth_transform
        self.pose_pred = MODELS.build(pose_head_cfg)
        self.flow_pred = XHead(self.h_channels, self.feat_channels, 2, x="flow")
        self.mask_pred = XHead(self.h_channels, self.feat_channels, 1, x="mask")
        mk = dict(conv_cfg=conv_cfg, norm_cfg=norm_cfg, act_cfg=act_cfg)
        self.delta_flow_encoder = nn.Sequential(
            ConvModule(2, 128, 7, padding=3, **mk), ConvModule(128, 64, 3, padding=1, **mk))
        self.mask_encoder = nn.Sequential(
            ConvModule(1, 64, 3, padding=1, **mk), ConvModule(64, 32, 3, padding=1, **mk))
        # name -> callable(start: bool) bracketing one launch (bench.py's live kernel timing):
        # gru_zr, gru_q, corr_pyramid, corr_lookup, pose_flow
        self.kernel_hooks: Dict[str, object] = {}
        # (hoist_context, tiled_pyramid, fuse_lookup_conv and fuse_lookup_conv_max_px: the shared
        # core's knobs, recurrent.py)
        # independent branches on a second HIP stream (else everything on the current stream)
        self.side_stream = True
        # the tail's flow-predictor / mask-predictor branches as paired launches on the main
        # stream (scflow_conv2d_pair) instead of two streams joined by events (round 6).
        # -1 = automatic: on for maps of at most 32 × 32 (configs[1]: 4.598 vs 4.612 ms per
        # forward, the profiled iteration 550 → 538 µs with 1.9 µs idle), off above (configs[4]:
        # 43.23 vs 43.17 ms) — profiles/r06/g11_*
        self.pair_tail = -1
        # the XHeads' predictors contracted in the hidden conv's epilogue (scflow_xhead_pred:
        # the 512-channel hidden output is never written; round 6) where the shapes allow it
        self.fuse_xhead_pred = os.environ.get("SCFLOW_XHEAD_PRED", "1") != "0"
        # fork / join with device-scope events (no system-scope cache writeback per record)
        self.device_scope_events = True
        # the iteration's tail (pose update, pose flow, ×8 prediction, next ↓8 flow) as one
        # launch (scflow_pose_step; under mask_flow scflow_pose_step_masked)
        self.fuse_tail = True
        # a batch of ≥ 2·pingpong_min pairs runs as two interleaved halves (_forward_pingpong).
        # Off: measured slower at B=16 (5.76 vs 5.33 ms/step) — a half's tail kernels do not get
        # CUs while the other half's convolutions hold every CU's LDS, so they serialise anyway
        self.pingpong = False
        self.pingpong_min = 4
        # with fuse_tail: the iteration's pose step runs only its ↓8 part (the next iteration's
        # flow, scflow_pose_step_part) on the critical path; its full-resolution outputs (pose
        # flow, ×8 prediction, mask) run on the side stream during the next iteration's GRU
        # (they only feed the returned lists)
        self.defer_full_res = True
        # with fuse_tail: the pose head's rotation / translation heads computed inside the pose
        # step's launch (scflow_pose_step_heads) instead of a launch of their own;
        # SCFLOW_FUSE_HEADS=0: off (A/B)
        self.fuse_heads = os.environ.get("SCFLOW_FUSE_HEADS", "1") != "0"
        # the deferred full-resolution part reads the pose the ↓8 part wrote instead of
        # recomputing the update per workgroup (ops.pose_step_given); SCFLOW_FULLRES_GIVEN=0: off
        self.fullres_given = os.environ.get("SCFLOW_FULLRES_GIVEN", "1") != "0"
        # 0: every stream at the default priority; 1: the forward's critical stream is a
        # high-priority stream of the decoder's own (the side branches at the default), so the
        # CP dispatches its workgroups first when both queues hold work; -1 (default): 1 for
        # feature maps above 32×32, else 0.  Measured (round 5, in-process A/B): configs[4]
        # 44.64 / 44.90 ms per forward for 1 / 0; configs[1] 4.926 / 4.841 ms — at 32² the side
        # branches are nearly as long as the critical ones and must not be held back
        self.main_priority = -1
        self._hooks_on = True
        self.hook_batch = 0

    # ------------------------------------------------------------------ helpers
    def _hidden_heads(self):
        """Both XHeads' first hidden conv as one launch when they have the same shape."""
        return super()._hidden_heads((("flow", self.flow_pred), ("mask", self.mask_pred)))

    def _xhead_pred_plan(self, head_runner, hid, HEAD, N, h, w, dev):
        """(hidden conv args, packed predictor weights, workspace, flow bias, mask bias) for
        scflow_xhead_pred, or None when the heads do not have its shape (3×3 two-output flow
        predictor, 1×1 one-output mask predictor, hidden convs on F(4×4,3×3), width 32 / 64)."""
        if not self.fuse_xhead_pred or head_runner is None or w not in (32, 64) or h % 4:
            return None
        fp, mp = self.flow_pred.predict_layer, self.mask_pred.predict_layer
        fh = self.flow_pred.layers[-1].conv.out_channels
        mh = self.mask_pred.layers[-1].conv.out_channels
        if (tuple(fp.kernel_size) != (3, 3) or tuple(fp.padding) != (1, 1) or tuple(fp.stride) != (1, 1)
                or fp.out_channels != 2 or tuple(mp.kernel_size) != (1, 1) or tuple(mp.padding) != (0, 0)
                or mp.out_channels != 1 or fh % 32 or mh % 32 or head_runner.act != "ReLU"):
            return None
        hargs = head_runner.args(hid, Chan.whole(HEAD), N, h, w)
        if hargs.bk != _lib.CONV_WINO4:
            return None
        pw = derived(self, "xhead_pred", (fp.weight, mp.weight),
                     lambda: ops.xhead_pred_pack(fp.weight, mp.weight))
        ws = ops.xhead_pred_workspace(N, h, w, fh, fh + mh, dev)
        fb = None if fp.bias is None else fp.bias.detach()
        mb = None if mp.bias is None else mp.bias.detach()
        return hargs, pw, ws, fb, mb, fh

    def _sync_events(self, dev, slot=0):
        """The fork / join events of a side stream (created once per device and slot, on it)."""
        evs = getattr(self, "_sync_evs", None)
        if evs is None:
            evs = self._sync_evs = {}
        if (dev, slot) not in evs:
            with torch.cuda.device(dev):
                evs[(dev, slot)] = (ops.SyncEvent(), ops.SyncEvent())
        return evs[(dev, slot)]

    def _pp_events(self, dev):
        """The two ping-pong events of _forward_pingpong (device scope, once per device)."""
        return self._sync_events(dev, "pingpong")

    def _side_stream(self, dev, slot=0) -> torch.cuda.Stream:
        """An extra HIP stream (created once per device and slot): slot 0 / 1 the side branches
        of each ping-pong half, "main1" the second half's main stream, "priority" (main_priority
        1) the critical stream at the highest priority the device allows (a lower number is a
        higher priority)."""
        ss = getattr(self, "_streams", None)
        if ss is None:
            ss = self._streams = {}
        if (dev, slot) not in ss:
            ss[(dev, slot)] = torch.cuda.Stream(device=dev, priority=-8 if slot == "priority" else 0)
        return ss[(dev, slot)]

    def _hook(self, name: str, start: bool) -> None:
        if not self._hooks_on:
            return
        h = self.kernel_hooks.get(name)
        if h is not None:
            h(start)

    def _hooks_for(self, *names):
        """Per-layer hooks for run_chain (None where no timer is installed); recorded with the
        segment's launches, so replays bracket the same launches."""
        if not self._hooks_on:
            return None
        hs = [self.kernel_hooks.get(n) if n else None for n in names]
        return hs if any(hs) else None

    # ------------------------------------------------------------------ forward
    def forward(self, feat_render: Tensor, feat_real: Tensor, h_feat: Tensor, cxt_feat: Tensor,
                ref_rotation: Tensor, ref_translation: Tensor, depth: Tensor, internel_k: Tensor,
                label: Tensor, init_flow: Tensor, invalid_flow_num: float,
                head_label: Optional[Tensor] = None):
        """``head_label`` (extension, default None = ``label``): the labels whose first entry
        picks the pose head's class for the whole batch (the reference's ``label[0]`` quirk,
        ``pose_head.py:208-209``).  A data-parallel shard passes the GLOBAL batch's ``label[:1]``
        so that sharded output equals the unsharded forward (``dist.shard_batch``)."""
        if feat_render.device.type != "cuda":
            raise ScflowError("SCFlowDecoder runs on the gfx950 HIP kernels only; move inputs to a "
                              "ROCm device (there is no CPU fallback)")
        with torch.no_grad():
            return self._forward(feat_render, feat_real, h_feat, cxt_feat, ref_rotation,
                                 ref_translation, depth, internel_k, label, init_flow,
                                 float(invalid_flow_num), head_label=head_label)

    def _forward(self, feat_render, feat_real, h_feat, cxt_feat, R0, t0, depth, K, label, init_flow,
                 invalid, hx: Optional[Tensor] = None, head_label: Optional[Tensor] = None):
        """``hx``: optional channels-last [N·h·w, ≥ hc+xc+co+2] buffer whose first hc+xc channels
        already hold tanh(h) | relu(cxt) (SCFlowRefiner writes the context encoder's output
        there directly); h_feat / cxt_feat are then ignored.

        With ``self.pingpong`` and a batch of ≥ 2·``pingpong_min`` pairs the batch runs as two
        halves interleaved on two stream pairs (``_forward_pingpong``); else as one."""
        args = (feat_render, feat_real, h_feat, cxt_feat, R0, t0, depth, K, label, init_flow, invalid)
        if self.pingpong and hx is None and feat_render.shape[0] >= 2 * self.pingpong_min:
            return self._forward_pingpong(*args, head_label)
        mp = self.main_priority
        if mp < 0:
            mp = 1 if feat_render.shape[-2] * feat_render.shape[-1] > 32 * 32 else 0
        if mp == 1:
            dev = feat_render.device
            cur = torch.cuda.current_stream(dev)
            hp = self._side_stream(dev, "priority")
            hp.wait_stream(cur)  # inputs produced on the caller's stream
            with torch.cuda.stream(hp):
                out = self._forward_single(*args, hx, head_label)
            cur.wait_stream(hp)
            _record_on(out, cur)
            return out
        return self._forward_single(*args, hx, head_label)

    def _forward_single(self, *args):
        """The whole batch as one run on the current stream (+ slot 0's side stream)."""
        run = _DecoderRun(self, *args)
        for it in range(run.iters):
            run.heavy(it)
            run.tail(it)
        run.finish()
        return run.lists()

    def _forward_pingpong(self, feat_render, feat_real, h_feat, cxt_feat, R0, t0, depth, K, label,
                          init_flow, invalid, head_label):
        """The batch as two halves A | B, each a complete run on its own (main, side) stream
        pair, with their iterations interleaved so that one half's latency-bound iteration tail
        (Δflow / mask encoders, pose head, pose update: many small launches that leave most CUs
        idle) runs while the other half's convolutions fill the chip.  Two device-scope events
        keep the halves' convolution phases ("heavy": lookup → motion encoder → GRU → heads) in
        strict alternation: A.heavy(i) → B.heavy(i) → A.heavy(i+1) → …, each half's tail
        overlapping the other's heavy phase.  Every sample is independent except the pose head's
        class, which both halves take from the whole batch's label[0] (pose_head.py:208-209), so
        the result equals the unsplit forward.  Outputs are written straight into the full-batch
        tensors (per-half views)."""
        dev = feat_render.device
        N = feat_render.shape[0]
        iters = int(self.iters)
        outs = _alloc_outputs(iters, N, *depth.shape[1:], self.pose_pred.rotation_out_channels, dev)
        gl = (label if head_label is None else head_label).to(dev).long()[:1]
        cur = torch.cuda.current_stream(dev)
        mains = [cur, self._side_stream(dev, "main1")]
        ev = self._pp_events(dev)  # (A heavy done, B heavy done)
        h_main = [m.cuda_stream for m in mains]
        mains[1].wait_stream(cur)  # inputs produced on the caller's stream

        def pp(k):
            def before(it):
                if k == 1:
                    ev[0].wait(h_main[1])      # B.heavy(i) after A.heavy(i)
                elif it > 0:
                    ev[1].wait(h_main[0])      # A.heavy(i) after B.heavy(i−1)

            def after(it):
                ev[k].record(h_main[k])
            return before, after

        runs = []
        for k, sl in enumerate((slice(0, N // 2), slice(N // 2, N))):
            with torch.cuda.stream(mains[k]):
                runs.append(_DecoderRun(
                    self, feat_render[sl], feat_real[sl], h_feat[sl], cxt_feat[sl], R0[sl], t0[sl],
                    depth[sl], K[sl], label[sl], init_flow[sl], invalid, head_label=gl,
                    outs={n: o[:, sl] for n, o in outs.items()}, slot=k, pp=pp(k), hooks=k == 0))
        # host issue order: A.heavy(i), B.heavy(i), A.tail(i), B.tail(i), …, each on its half's
        # main stream
        for it in range(iters):
            for phase in (_DecoderRun.heavy, _DecoderRun.tail):
                for k in (0, 1):
                    with torch.cuda.stream(mains[k]):
                        phase(runs[k], it)
        for k in (0, 1):
            with torch.cuda.stream(mains[k]):
                runs[k].finish()
        cur.wait_stream(mains[1])
        return _lists(outs)


class _DecoderRun:
    """One forward (or one ping-pong half) on the stream that is current when it is built, plus
    ``slot``'s side stream: the shared ``RecurrentCore``, the buffers of what follows the GRU, the
    plan, the ``_Streams`` and the stacked outputs.  The caller drives ``heavy(it)`` and
    ``tail(it)`` for every iteration, then ``finish()``; ``lists()`` is the 7-list return.

    ``outs``: preallocated stacked outputs (``_forward_pingpong``'s per-half views); ``pp``:
    (before(it), after(it)) callables that order this half's heavy phase against the other's;
    ``hooks``: whether the bench's kernel timers bracket this run's launches.

    Host path: the launches that read and write the same persistent buffers in every iteration
    are recorded on the first iteration (``core.segment`` / ``ops.binding``: argument structs built
    once) and replayed afterwards as one ctypes call each; the launches whose pointers change per
    iteration (poses, outputs) have their calls for every iteration built once
    (``build_tail_calls``).  This keeps the host well ahead of the GPU (a Python wrapper costs
    more than several of the pose head's kernels take to run).

    Every buffer is allocated on the main stream and outlives the forward, and the main stream
    always waits for the side stream before they are reused.  Buffers written in one iteration
    and read during the next come in pairs indexed by the iteration's parity (``_at``): the ↓8
    flow F2 under the fused tail (its launch writes the next iteration's), Δflow and the mask when
    the full-resolution outputs are deferred.  Under occlusion masking (mask_corr / mask_flow,
    scflow_decoder.py:189-207) the mask the previous iteration predicted (all ones before the
    first) scales the correlation samples inside the lookup kernels (mask_corr) and the ↓8 flow
    inside the launch that produces it (mask_flow: the tail, or the downsample): F2 stays the
    unmasked flow (the lookup's centroids), FLM = F2 · mask feeds the flow branch and the motion
    features' flow channels, buffered like F2."""

    def __init__(self, dec: SCFlowDecoder, feat_render, feat_real, h_feat, cxt_feat, R0, t0, depth,
                 K, label, init_flow, invalid, hx: Optional[Tensor] = None,
                 head_label: Optional[Tensor] = None, outs: Optional[dict] = None, slot=0, pp=None,
                 hooks: bool = True) -> None:
        self.dec, self.pp, self.hooks, self.invalid = dec, pp, hooks, invalid
        dev = feat_render.device
        dec._hooks_on = hooks
        dec.hook_batch = feat_render.shape[0]  # pairs per bracketed launch (bench roofline)
        feat_render = feat_render.contiguous().float()
        feat_real = feat_real.contiguous().float()
        N, _, h, w = feat_render.shape
        self.N, self.h, self.w = N, h, w
        self.H, self.W = depth.shape[1:]
        self.scale = 2 ** (dec.num_levels - 1)
        self.iters = iters = int(dec.iters)
        # a1 + a9 (once per forward), then the channels-last working set; the motion encoder's
        # and the GRU's buffers and launches are the shared core's (recurrent.py)
        self.core = core = RecurrentCore(dec, feat_render, feat_real, dec._hook, dec._hooks_for)
        self.K = K.contiguous().float()
        self.R_prev, self.t_prev = R0.contiguous().float(), t0.contiguous().float()
        self.points = ops.lift_points(depth.contiguous().float(), self.K, self.R_prev, self.t_prev)
        core.bind_state(h_feat, cxt_feat, hx)
        self.label = (label if head_label is None else head_label).to(dev).long()
        self.flow_full = init_flow.contiguous().float()
        self.out = outs if outs is not None else _alloc_outputs(
            iters, N, self.H, self.W, dec.pose_pred.rotation_out_channels, dev)
        self.st = _Streams.of(dec, dev, slot)

        # the plan (last_plan's keys; the mask flags do not change it)
        self.masked = bool(dec.mask_corr or dec.mask_flow)
        self.fuse_tail = fuse_tail = bool(dec.fuse_tail)
        self.defer = defer = bool(fuse_tail and dec.defer_full_res and iters > 1)
        pt = dec.pair_tail if dec.pair_tail >= 0 else int(h * w <= 32 * 32)
        self.pair_tail = bool(pt) and len(dec.delta_flow_encoder) == len(dec.mask_encoder)
        self.mark = defer and self.pair_tail  # the mark / wait pair of the deferred launches (tail)
        dec._last_plan = dict(fuse_tail=fuse_tail, defer=defer, pair_tail=self.pair_tail,
                              fuse_lc=core.fuse_lc, tiled=core.tiled, side_stream=self.st.two)
        if core.gru_bf16:
            dec._last_plan["gru_bf16"] = True
        if core.menc_bf16:
            dec._last_plan["menc_bf16"] = True

        def bufs(channels, two):
            return [torch.empty(core.M, channels, device=dev, dtype=torch.float32)
                    for _ in range(2 if two else 1)]
        self.fh = fh = dec.flow_pred.layers[-1].conv.out_channels
        self.mh = mh = dec.mask_pred.layers[-1].conv.out_channels
        self.dfc = dfc = dec.delta_flow_encoder[-1].conv.out_channels
        self.mfc = mfc = dec.mask_encoder[-1].conv.out_channels
        self.HEAD = bufs(fh + mh, False)[0]
        self.FM = bufs(dfc + mfc, False)[0]  # [Δflow feat | mask feat]
        self.s_dfe = core.scratch(dec.delta_flow_encoder)
        self.s_me = core.scratch(dec.mask_encoder)
        self.F2s = bufs(2, fuse_tail)
        self.FLMs = bufs(2, fuse_tail) if dec.mask_flow else self.F2s
        self.D2s, self.MASKs = bufs(2, defer), bufs(1, defer)
        if self.masked:  # before the first prediction: interpolate(ones, 1/8) == ones
            _at(self.MASKs, -1).fill_(1.0)
        if defer:  # the deferred launches' pose outputs (duplicates of the outputs: not read)
            self.R_scr = torch.empty(N, 3, 3, device=dev, dtype=torch.float32)
            self.t_scr = torch.empty(N, 3, device=dev, dtype=torch.float32)
        self.head_runner = dec._hidden_heads()
        self.flow_pred_r = ConvRunner.of(dec.flow_pred.predict_layer, None)
        self.mask_pred_r = ConvRunner.of(dec.mask_pred.predict_layer, "Sigmoid")
        self.xpred = dec._xhead_pred_plan(self.head_runner, core.hid, self.HEAD, N, h, w, dev)
        self.keep = []  # buffers the recorded pose-head launches write (alive for the forward)
        self.pose_x = None  # the pose trunk's output (set when its launches are recorded)
        self.tail_calls = None  # fused tail: per-iteration (heads, pose step, deferred) launches
        self.pending = []  # the previous iteration's deferred full-resolution launches
        self.par = 0

    # ------------------------------------------------------------------ the two phases
    def heavy(self, it: int) -> None:
        """The ↓8 flow through the heads: the phase whose convolutions fill the chip."""
        dec, core, st = self.dec, self.core, self.st
        dec._hooks_on = self.hooks
        self.par = it % 2
        sfx = str(self.par) if self.fuse_tail else ""  # recorded once per F2 buffer
        F2, flow_in = _at(self.F2s, it), _at(self.FLMs, it)
        # the mask iteration it−1 predicted (ones before the first)
        mask_prev = _at(self.MASKs, it - 1) if self.masked else None
        # a11 ↓: flow at feature resolution → F2 (and the motion-feature flow channels, times
        # the mask under mask_flow); the fused tail of the previous iteration already wrote it
        if not self.fuse_tail or it == 0:
            masked = dict(mask=mask_prev, outm=Chan.whole(flow_in)) if dec.mask_flow else {}
            ops.flow_downsample(self.flow_full, Chan.whole(F2), self.h, self.w, 1.0 / self.scale,
                                out1=core.hx_flow, **masked)
        if self.pp is not None:
            self.pp[0](it)
        # a3 (flow branch) on the side stream ‖ a2 + a3 (correlation branch)
        st.fork()
        with torch.cuda.stream(st.side):
            core.flow_branch(sfx, flow_in)
        core.correlation(sfx, F2, mask_prev if dec.mask_corr else None)
        st.join()
        if self.pending:
            # the previous iteration's full-resolution outputs on the side stream AFTER the
            # join's record: they overlap out_net and the GRU (MFMA-bound) instead of
            # lengthening a joined branch (what orders their inputs: see tail)
            with torch.cuda.stream(st.side):
                dec._hook("pose_flow", True)
                for c in self.pending:
                    c()
                dec._hook("pose_flow", False)
                if self.mark:
                    st.mark_side()
            self.pending = []
        core.motion_out()
        core.gru(dec.kernel_hooks)  # a4, in place on HX[:, :hc]
        # a5 heads (with xpred: the predictors too, into this iteration's Δflow / mask)
        dec._hook("heads", True)
        core.segment("heads" + (sfx if self.xpred is not None and self.defer else ""), self.seg_heads)
        dec._hook("heads", False)
        if self.pp is not None:
            self.pp[1](it)

    def tail(self, it: int) -> None:
        """The tail branches through the pose step: many small, latency-bound launches.

        Deferred outputs: iteration j's deferred launch is queued on the side stream in
        heavy(j+1), behind its join, and reads F2s[j % 2], D2s[j % 2] and MASKs[j % 2] (the flow
        branch, earlier on that stream, read FLMs[j % 2]).  Each one's next writer is ordered
        after it.  F2s / FLMs[j % 2]: iteration j+1's pose step on the main stream (its
        lr_next / lrm_next) — the unpaired tail's join precedes it; under the paired tail no join
        does, so heavy(j+1) marks the side stream after the deferred launch and the pose step
        waits for that mark.  D2s / MASKs[j % 2]: iteration j+2's predictors, on the main stream
        after heavy(j+2)'s join, or (unpaired mask branch) on the side stream itself."""
        dec, core, st, out = self.dec, self.core, self.st, self.out
        dec._hooks_on = self.hooks
        sfx = str(self.par) if self.defer else ""  # recorded once per Δflow / mask buffer
        if self.pair_tail:
            # flow predictor + Δflow encoder ‖ mask predictor + mask encoder (a5, a6) as paired
            # launches on this stream
            core.segment("tail_pair" + sfx, self.seg_tail_pair)
        else:
            # mask predictor + mask encoder on the side stream (the shorter branch), flow
            # predictor + Δflow encoder on this one
            st.fork()
            with torch.cuda.stream(st.side):
                core.segment("mask_branch" + sfx, self.seg_mask_branch)
            core.segment("flow_pred" + sfx, self.seg_flow_pred)
            st.join()
        # a7 pose head on cat[h, Δflow feat, mask feat] (two channel sources, no concat)
        core.segment("pose_trunk", self.seg_pose_trunk)
        if self.fuse_tail:
            # a8 + a10 + a11 ↑ (+ the next iteration's a11 ↓): one launch, replayed from the
            # calls built after the trunk's first pass
            if self.tail_calls is None:
                self.tail_calls = self.build_tail_calls()
            hc, pc, fc = self.tail_calls[it]
            for c in hc:
                c()
            if self.mark and it > 0:  # after iteration it−1's deferred launch
                st.wait_side_mark()
            # deferred: this is the critical-path ↓8 launch (its own timer); otherwise the
            # whole pose step
            hook = "pose_step_crit" if fc else "pose_flow"
            dec._hook(hook, True)
            for c in pc:
                c()
            dec._hook(hook, False)
            if dec.kernel_hooks:  # measurement only: bench.py times a launch alone
                dec._tail_calls = self.tail_calls
            self.pending = fc
        else:
            dec.pose_pred.heads_hip(self.pose_x, self.label, out["drot"][it], out["dt"][it])
            # a11 ↑: flow_pred = 8·up(flow + Δflow), mask ↑
            ops.flow_upsample(_at(self.F2s, it), self.D2s[0], self.MASKs[0], self.N, self.h, self.w,
                              self.H, self.W, float(self.scale), out["flow_pred"][it], out["mask"][it])
            # a8 + a10: pose update + pose-induced flow (one launch)
            dec._hook("pose_flow", True)
            ops.pose_update_flow(out["drot"][it], out["dt"][it], self.R_prev, self.t_prev, self.K,
                                 self.points, out["R"][it], out["t"][it], out["flow_pose"][it],
                                 self.invalid, depth_transform=dec.depth_transform)
            dec._hook("pose_flow", False)
            # (the fused tail's launches hold every iteration's pointers already)
            self.R_prev, self.t_prev = out["R"][it], out["t"][it]
            self.flow_full = out["flow_pose"][it]

    def finish(self) -> None:
        """With the tail paired on the main stream the side stream's last work (the deferred
        full-resolution outputs queued in the last iteration) is not joined inside the loop."""
        if self.pair_tail:
            self.st.join()

    def lists(self):
        return _lists(self.out)

    # ------------------------------------------------------------------ the recorded segments
    def seg_heads(self):
        dec, core = self.dec, self.core
        if self.xpred is not None:  # hidden conv + both predictors → Δflow, mask
            hargs, pw, xws, fb, mb, fh_ = self.xpred
            ops.xhead_pred(hargs, fh_, pw, xws, fb, mb, None, "Sigmoid",
                           Chan.whole(_at(self.D2s, self.par)), Chan.whole(_at(self.MASKs, self.par)))
        elif self.head_runner is not None:
            self.head_runner.run(core.hid, Chan.whole(self.HEAD), self.N, self.h, self.w)
        else:
            run_chain(dec.flow_pred.layers, core.hid, Chan(self.HEAD, 0, self.fh), self.N, self.h, self.w)
            run_chain(dec.mask_pred.layers, core.hid, Chan(self.HEAD, self.fh, self.mh), self.N,
                      self.h, self.w)

    def seg_mask_branch(self):
        N, h, w, MK = self.N, self.h, self.w, _at(self.MASKs, self.par)
        if self.xpred is None:
            self.mask_pred_r.run(Chan(self.HEAD, self.fh, self.mh), Chan.whole(MK), N, h, w)
        run_chain(self.dec.mask_encoder, Chan.whole(MK), Chan(self.FM, self.dfc, self.mfc), N, h, w,
                  self.s_me, hooks=self.dec._hooks_for(None, "mask_enc1"))

    def seg_tail_pair(self):
        # the flow-predictor and mask-predictor branches on the main stream, their k-th
        # launches paired into one grid each (scflow_conv2d_pair): no fork / join events
        N, h, w, HEAD, FM = self.N, self.h, self.w, self.HEAD, self.FM
        D2, MK = _at(self.D2s, self.par), _at(self.MASKs, self.par)
        if self.xpred is None:
            ops.conv2d_pair(
                self.flow_pred_r.args(Chan(HEAD, 0, self.fh), Chan.whole(D2), N, h, w),
                self.mask_pred_r.args(Chan(HEAD, self.fh, self.mh), Chan.whole(MK), N, h, w), HEAD)
        run_chain_pair(self.dec.delta_flow_encoder, Chan.whole(D2), Chan(FM, 0, self.dfc),
                       self.dec.mask_encoder, Chan.whole(MK), Chan(FM, self.dfc, self.mfc), N, h, w,
                       self.s_dfe, self.s_me)

    def seg_flow_pred(self):
        N, h, w, D2 = self.N, self.h, self.w, _at(self.D2s, self.par)
        if self.xpred is None:
            self.flow_pred_r.run(Chan(self.HEAD, 0, self.fh), Chan.whole(D2), N, h, w)
        run_chain(self.dec.delta_flow_encoder, Chan.whole(D2), Chan(self.FM, 0, self.dfc), N, h, w,
                  self.s_dfe, hooks=self.dec._hooks_for(None, "dflow1"))

    def seg_pose_trunk(self):
        self.pose_x = self.dec.pose_pred.trunk_hip(self.core.hid, Chan.whole(self.FM), self.N,
                                                   self.h, self.w, ws=self.keep)

    def build_tail_calls(self):
        """The fused tail's launches for every iteration, one (heads, pose step, deferred
        full-resolution) tuple of call lists each: they take per-iteration pointers, so their
        argument structs are built once (after the trunk's first pass) and replayed."""
        dec, out, iters = self.dec, self.out, self.iters
        F2s, FLMs, D2s, MASKs = self.F2s, self.FLMs, self.D2s, self.MASKs
        calls = []
        Rp, tp = self.R_prev, self.t_prev
        for j in range(iters):
            last = j == iters - 1
            hc, pc, fc = [], [], []
            # what every variant of the iteration's launch shares: the full-resolution part
            full = dict(K=self.K, points=self.points, flow_out=out["flow_pose"][j],
                        invalid_num=self.invalid, lr=_at(F2s, j), delta=_at(D2s, j),
                        mask=_at(MASKs, j), flow_up=out["flow_pred"][j], mask_up=out["mask"][j],
                        h=self.h, w=self.w, up_scale=float(self.scale))
            # the pose update from this iteration's delta
            upd = dict(drot=out["drot"][j], dt=out["dt"][j], R=Rp, t=tp, R_out=out["R"][j],
                       t_out=out["t"][j], depth_transform=dec.depth_transform)
            # the next iteration's ↓8 flow (under mask_flow: and its masked copy)
            nxt = {} if last else dict(lr_next=Chan.whole(_at(F2s, j + 1)), hx_next=self.core.hx_flow)
            if dec.mask_flow and not last:
                nxt.update(mask_next=_at(MASKs, j), lrm_next=Chan.whole(_at(FLMs, j + 1)))
            # the rotation / translation heads inside the pose step's launch, or as their own
            # launch before it
            ha = dec.pose_pred.heads_args(self.pose_x, self.label) if dec.fuse_heads else None
            if ha is None:
                with ops.binding(hc, run=False):
                    dec.pose_pred.heads_hip(self.pose_x, self.label, out["drot"][j], out["dt"][j])
            heads = {} if ha is None else dict(heads=ha)
            if self.defer and not last:
                with ops.binding(pc, run=False):  # critical: only the ↓8 flow
                    ops.pose_step(**full, **upd, **nxt, **heads, parts=2)
                with ops.binding(fc, run=False):  # deferred: only the full-resolution part
                    if dec.fullres_given:  # from the pose the ↓8 launch wrote
                        ops.pose_step_given(R=out["R"][j], t=out["t"][j], **full)
                    else:  # the update again, from the deltas the ↓8 launch wrote
                        ops.pose_step(**full, **dict(upd, R_out=self.R_scr, t_out=self.t_scr),
                                      lr_next=nxt["lr_next"], hx_next=nxt["hx_next"], parts=1)
            else:
                with ops.binding(pc, run=False):
                    ops.pose_step(**full, **upd, **nxt, **heads)
            calls.append((hc, pc, fc))
            Rp, tp = out["R"][j], out["t"][j]
        return calls
