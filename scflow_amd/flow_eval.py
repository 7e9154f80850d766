"""Flow validation on the device: the GT flow with its validity filters, the end-point error (EPE)
with its 1 / 3 / 5 px accuracies and the occlusion error — what the refiners' ``val_step`` reports.

Reference: ``models/utils/pose.py:92-121`` (``get_flow_from_delta_pose_and_depth``),
``models/utils/flow.py:6-88`` (``filter_flow_by_mask``, ``filter_flow_by_depth``,
``filter_flow_by_face_index``, ``cal_epe``) and ``models/refiner/raft_refiner_flow_mask.py:239-259``
(``eval_epe_and_occ``).  Two HIP entry points do the work: ``scflow_flow_gt`` — the
flow and all its filters in one launch — and ``scflow_flow_epe`` — the per-sample statistics
without an ``[N, H, W]`` intermediate, bitwise reproducible.  Nothing here synchronises with the
host; there is no CPU path.

Deliberate deviations from the reference, all three documented in INTEGRATION.md:

* Every function is OUT OF PLACE.  The reference's filters write into the flow they are given
  (and return it); here the input keeps its values and the filtered flow is a new tensor.
* ``filter_flow_by_depth`` combines as ``not_valid | ~consistent`` by default (``combine='or'``):
  it invalidates depth-inconsistent pixels, as the LoFTR code it cites and the other two filters
  do.  The reference writes ``not_valid & ~consistent``, which can only rewrite pixels that are
  invalid already — a no-op on a freshly built GT flow; ``combine='reference'`` is that expression
  exactly.
* ``cal_epe(reduction='mean')`` returns the per-sample accuracies over the VALID pixels.  The
  reference's branch overwrites the valid errors with 1e8 before thresholding (flow.py:79), so its
  ``…px`` entries count the invalid pixels instead; its ``'mean'`` entry is the reference's.

Statistics are float64 tensors: they are fp64 sums of the fp32 per-pixel errors divided by the
integer counts (the reference divides by ``count + 1e-10``; so does this, which turns a sample
without a valid pixel into zeros instead of NaN).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import library  # noqa: F401  (registers torch.ops.scflow.flow_gt / flow_epe)

Tensor = torch.Tensor

_EPS = 1e-10  # flow.py:77, 84


def _f32(x: Tensor) -> Tensor:
    return x.contiguous().float()


def _mask_arg(m: Optional[Tensor]) -> Optional[Tensor]:
    """A mask the kernel reads as it is (bool / uint8 / float32); anything else as float32."""
    if m is None:
        return None
    m = m.contiguous()
    return m if m.dtype in (torch.bool, torch.uint8, torch.float32) else m.float()


def _face_arg(f: Optional[Tensor]) -> Optional[Tensor]:
    if f is None:
        return None
    f = f.contiguous()
    return f if f.dtype in (torch.int32, torch.int64) else f.long()


def gt_flow(depth: Tensor, K: Tensor, R_ref: Tensor, t_ref: Tensor, R_gt: Tensor, t_gt: Tensor,
            invalid_num: float = 400., gt_mask: Optional[Tensor] = None,
            gt_depth: Optional[Tensor] = None, depth_thr: float = 0.2, depth_combine: str = "or",
            face_index: Optional[Tensor] = None, gt_face_index: Optional[Tensor] = None
            ) -> Tuple[Tensor, Tensor]:
    """The GT flow of a rendered depth [N, H, W] between the reference pose and the GT pose
    (``get_flow_from_delta_pose_and_depth``; the bits of ``ops.lift_points`` + ``ops.pose_flow``)
    and the same flow with the selected filters applied, in ONE launch → (flow, filtered flow),
    both [N, 2, H, W]; invalid pixels hold ``invalid_num`` in both channels.

    ``gt_mask`` [N, H, W] (bool / uint8 / float): ``filter_flow_by_mask``.  ``gt_depth`` [N, H, W],
    the depth rendered at the GT pose: ``filter_flow_by_depth`` with ``depth_thr`` and
    ``depth_combine`` ('or', the default, or 'reference': see the module docstring).
    ``face_index`` / ``gt_face_index`` [N, H, W] (the int64 ``pix_to_face`` of ``Fragments`` as it
    is, or int32): ``filter_flow_by_face_index``.  Each filter decides from the unfiltered flow,
    which equals applying them one after another.  Without a filter the second tensor is a copy."""
    fi, gfi = _face_arg(face_index), _face_arg(gt_face_index)
    if fi is not None and gfi is not None and gfi.dtype != fi.dtype:
        fi, gfi = fi.long(), gfi.long()
    return torch.ops.scflow.flow_gt(
        _f32(depth), _f32(K), _f32(R_ref), _f32(t_ref), _f32(R_gt), _f32(t_gt), None,
        float(invalid_num), _mask_arg(gt_mask), None if gt_depth is None else _f32(gt_depth),
        float(depth_thr), depth_combine, fi, gfi)


def _filter(flow: Tensor, invalid_num: float, **kw) -> Tensor:
    args = dict(gt_mask=None, depth0=None, depth1=None, thr=0.2, combine="or", f1=None, f2=None)
    args.update(kw)
    _, out = torch.ops.scflow.flow_gt(
        args["depth0"], None, None, None, None, None, _f32(flow), float(invalid_num),
        args["gt_mask"], args["depth1"], float(args["thr"]), args["combine"], args["f1"], args["f2"])
    return out


def filter_flow_by_mask(flow: Tensor, gt_mask: Tensor, invalid_num: float = 400,
                        mode: str = "bilinear", align_corners: bool = False) -> Tensor:
    """flow.py:6-26 — flow [N, 2, H, W] from the source to the target image, gt_mask [N, H, W] the
    target's mask: a pixel is invalid where the mask sampled at its target (bilinear, zero padding,
    the reference's coordinates) is < 0.9 or both channels are ≥ ``invalid_num``.  Returns a NEW
    tensor (the reference writes into ``flow``).  Only the reference's defaults of ``mode`` and
    ``align_corners`` — the values every caller uses — are built."""
    if mode != "bilinear" or align_corners:
        raise NotImplementedError("filter_flow_by_mask: mode='bilinear', align_corners=False only "
                                  "(the reference's defaults, which all its callers use)")
    return _filter(flow, invalid_num, gt_mask=_mask_arg(gt_mask))


def filter_flow_by_depth(flow: Tensor, depth1: Tensor, depth0: Tensor, invalid_num: float = 400,
                         thr: float = 0.2, combine: str = "or") -> Tensor:
    """flow.py:28-45 — flow from image 0 to image 1, their depths [N, H, W]: depth1 warped to image
    0 (bilinear, align_corners=True, zero padding, non-positive depths zeroed) is consistent where
    ``|depth0 − warped| / (depth0 + 0.1) < thr``.  ``combine='or'`` (default) invalidates the
    inconsistent pixels; ``combine='reference'`` is the reference's ``&`` (module docstring).
    Returns a NEW tensor."""
    return _filter(flow, invalid_num, depth0=_f32(depth0), depth1=_f32(depth1), thr=thr,
                   combine=combine)


def filter_flow_by_face_index(flow: Tensor, face_index1: Tensor, face_index2: Tensor,
                              invalid_num: float = 400) -> Tensor:
    """flow.py:47-59 — a pixel is invalid where ``face_index2`` sampled at its target (nearest, ties
    to even, align_corners=True, zero padding) differs from ``face_index1``, or where the flow is
    invalid already.  Indices are compared as float32, as the reference converts them.  Returns a
    NEW tensor."""
    f1, f2 = _face_arg(face_index1), _face_arg(face_index2)
    if f1.dtype != f2.dtype:
        f1, f2 = f1.long(), f2.long()
    return _filter(flow, invalid_num, f1=f1, f2=f2)


def flow_stats(flow_tgt: Tensor, flow_pred: Tensor, mask: Optional[Tensor] = None,
               max_flow: float = 400, threshs: Sequence[float] = (1, 3, 5),
               occ_pred: Optional[Tensor] = None, error_map: bool = False) -> Dict[str, Tensor]:
    """The raw per-sample statistics, device tensors, no synchronisation: ``count`` [N] int32 (the
    valid pixels: ``|flow_tgt| < max_flow``, and ``mask ≥ 0.5`` where a mask is given), ``below``
    [N, 3] int32 (the valid pixels whose error is below each threshold), ``err_sum`` [N] float64,
    ``occ_sum`` [N] float64 (Σ over all pixels of ``|(|flow_tgt| < max_flow) − occ_pred|``; only
    with ``occ_pred`` [N, H, W] or [N, 1, H, W]), ``num_pixels`` (H·W, an int) and, with
    ``error_map``, ``error_map`` [N, H, W].  Counts are exact and sums bitwise reproducible."""
    tgt = _f32(flow_tgt)
    n, _, h, w = tgt.shape
    occ = None if occ_pred is None else _f32(occ_pred).reshape(n, h, w)
    m = None if mask is None else _f32(mask).reshape(n, h, w)
    counts, sums, emap = torch.ops.scflow.flow_epe(tgt, _f32(flow_pred), m, float(max_flow),
                                                   [float(v) for v in threshs], occ, error_map, True)
    out = dict(count=counts[:, 0], below=counts[:, 1:], err_sum=sums[:, 0], num_pixels=h * w)
    if occ is not None:
        out["occ_sum"] = sums[:, 1]
    if error_map:
        out["error_map"] = emap
    return out


def _total_mean(st: Dict[str, Tensor], threshs) -> "OrderedDict[str, Tensor]":
    total = st["count"].sum().double() + _EPS
    acc = OrderedDict(mean=st["err_sum"].sum() / total)
    below = st["below"].sum(0).double()
    for k, thr in enumerate(threshs):
        acc[f"{thr}px"] = below[k] / total
    return acc


def cal_epe(flow_tgt: Tensor, flow_pred: Tensor, mask: Optional[Tensor], max_flow: float = 400,
            reduction: str = "mean", threshs: Sequence[float] = (1, 3, 5)):
    """flow.py:64-88.  ``'none'``: the error map [N, H, W], zero at invalid pixels (one launch).
    ``'total_mean'``: the dict ``mean``, ``1px``, ``3px``, ``5px`` over the whole batch (0-dim
    float64 tensors) — what the reference's ``val_step`` uses.  ``'mean'``: the same keys as [N]
    tensors per sample; the ``…px`` entries are the accuracies over the valid pixels, NOT the
    reference's (module docstring), ``mean`` is the reference's.  Exactly three thresholds."""
    if reduction not in ("none", "mean", "total_mean"):
        raise ValueError(f"reduction = {reduction!r}: 'none', 'mean' or 'total_mean'")
    threshs = tuple(threshs)
    if reduction == "none":
        tgt = _f32(flow_tgt)
        n, _, h, w = tgt.shape
        m = None if mask is None else _f32(mask).reshape(n, h, w)
        return torch.ops.scflow.flow_epe(tgt, _f32(flow_pred), m, float(max_flow),
                                         [float(v) for v in threshs], None, True, False)[2]
    return _reduce(flow_stats(flow_tgt, flow_pred, mask, max_flow, threshs), reduction, threshs)


def _reduce(st: Dict[str, Tensor], reduction: str, threshs) -> "OrderedDict[str, Tensor]":
    if reduction == "total_mean":
        return _total_mean(st, threshs)
    total = st["count"].double() + _EPS
    acc = OrderedDict(mean=st["err_sum"] / total)
    for k, thr in enumerate(threshs):
        acc[f"{thr}px"] = st["below"][:, k].double() / total
    return acc


def eval_epe_and_occ(batch_flow: Tensor, batch_occlusion: Optional[Tensor], rendered_depths: Tensor,
                     gt_rotations: Tensor, gt_translations: Tensor, internel_k: Tensor,
                     ref_rotations: Tensor, ref_translations: Tensor, gt_masks: Optional[Tensor],
                     max_flow: float = 400., reduction: str = "mean",
                     noc_without_mask: bool = False) -> "OrderedDict[str, Tensor]":
    """raft_refiner_flow_mask.py:239-259 with the reference's keys — ``epe_mean``, ``epe_1px``,
    ``epe_3px``, ``epe_5px`` against the GT flow, ``epe_noc_*`` against the GT flow filtered by
    ``gt_masks`` (only with ``gt_masks``), ``occ`` = the mean over the batch's pixels of
    ``|(|noc GT flow| < max_flow) − batch_occlusion|`` (only with ``batch_occlusion``; the
    reference's method always has one).  One ``scflow_flow_gt`` launch and two ``scflow_flow_epe``
    launches (one without ``gt_masks``), no synchronisation: the values are device tensors.
    ``reduction``: 'mean' (per sample, see ``cal_epe``) or 'total_mean'; ``occ`` is the batch mean
    in both.  ``noc_without_mask``: without ``gt_masks`` repeat the ``epe_*`` values as
    ``epe_noc_*`` (base_flow_refiner.py:94-95, the plain RAFT refiner's behaviour)."""
    flow, noc = gt_flow(rendered_depths, internel_k, ref_rotations, ref_translations, gt_rotations,
                        gt_translations, invalid_num=max_flow, gt_mask=gt_masks)
    return epe_and_occ_against(flow, noc if gt_masks is not None else None, batch_flow,
                               batch_occlusion, max_flow, reduction, noc_without_mask)


def epe_and_occ_against(flow: Tensor, noc_flow: Optional[Tensor], batch_flow: Tensor,
                        batch_occlusion: Optional[Tensor] = None, max_flow: float = 400.,
                        reduction: str = "mean", noc_without_mask: bool = False,
                        prefix: str = "epe") -> "OrderedDict[str, Tensor]":
    """``eval_epe_and_occ`` against a GT flow that is already there (``gt_flow``'s pair; ``noc_flow``
    None: no GT mask): the ``scflow_flow_epe`` launches alone, so one GT flow serves several
    predictions.  Keys ``{prefix}_*``, ``{prefix}_noc_*`` and, with ``batch_occlusion``, ``occ``."""
    if reduction not in ("mean", "total_mean"):
        raise ValueError(f"reduction = {reduction!r}: 'mean' or 'total_mean'")
    threshs = (1, 3, 5)
    with_noc = noc_flow is not None
    metric = OrderedDict()
    st = flow_stats(flow, batch_flow, None, max_flow, threshs,
                    occ_pred=None if with_noc else batch_occlusion)
    epe = _reduce(st, reduction, threshs)
    for k, v in epe.items():
        metric[f"{prefix}_{k}"] = v
    occ_st = st
    if with_noc:
        occ_st = flow_stats(noc_flow, batch_flow, None, max_flow, threshs, occ_pred=batch_occlusion)
        for k, v in _reduce(occ_st, reduction, threshs).items():
            metric[f"{prefix}_noc_{k}"] = v
    elif noc_without_mask:
        for k, v in epe.items():
            metric[f"{prefix}_noc_{k}"] = v
    if batch_occlusion is not None:
        metric["occ"] = occ_st["occ_sum"].sum() / float(occ_st["count"].shape[0] * occ_st["num_pixels"])
    return metric


def log_vars(metric: "OrderedDict[str, Tensor]") -> "OrderedDict[str, float]":
    """0-dim device statistics → floats with ONE host synchronisation (``val_step``'s log_vars)."""
    host = torch.stack([v.double().reshape(()) for v in metric.values()]).tolist()
    return OrderedDict(zip(metric.keys(), host))
