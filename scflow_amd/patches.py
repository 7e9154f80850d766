"""Patches from full frames on the device: crop, resize, pad and the adapted intrinsics.

Reference: the test pipeline ``ComputeBbox → Crop → Resize(keep_ratio) → Pad(center) →
RemapPose(adapt_intrinsic) → Normalize`` (``datasets/pipelines/formatting.py:42-91``,
``geometry_transform.py:155-500``, ``configs/refine_datasets/ycbv_real.py:76-99``), which runs per
object on the host with cv2 / mmcv.  Here it is two HIP launches for all objects of a batch
(``ops.patch_boxes``, ``ops.extract_patches``; DESIGN.md §15 states the geometry) with no host
synchronisation: the crop sizes stay in device memory.  Image decoding stays the caller's.

In ``adapt_intrinsic`` mode the pose is unchanged by the crop (``models/utils/pose.py:275-277``):
a pose refined on the patches under ``internel_k`` is the pose in the original camera.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import torch

from . import ops
from ._lib import ScflowError

Tensor = torch.Tensor

# configs/refine_datasets/ycbv_real.py:12-13, :87
IMG_NORM_CFG = dict(mean=(0.0, 0.0, 0.0), std=(255.0, 255.0, 255.0))


def point_table(renderer) -> Tuple[Tensor, Tensor]:
    """(points [C, P, 3] float32, counts [C] int32) from the meshes a ``Renderer`` holds, on their
    device: class ``l`` owns ``points[l, :counts[l]]`` — ALL vertices of its mesh; a label without
    a mesh has count 0 (its objects come out invalid).  The reference's ``ComputeBbox`` draws 1000
    random vertices of ``models_eval`` instead (formatting.py:53-55), so its boxes are at most as
    large as these and differ from run to run."""
    if not renderer.meshes:
        raise ScflowError("point_table: the renderer holds no mesh")
    c = max(renderer.meshes) + 1
    p = max(m[0].shape[0] for m in renderer.meshes.values())
    dev = next(iter(renderer.meshes.values()))[0].device
    points = torch.zeros(c, p, 3, device=dev, dtype=torch.float32)
    counts = torch.zeros(c, dtype=torch.int32)
    for lab, m in renderer.meshes.items():
        points[lab, :m[0].shape[0]] = m[0]
        counts[lab] = m[0].shape[0]
    return points, counts.to(dev)


def _i32(x: Tensor) -> Tensor:
    return x.contiguous().to(torch.int32)


def frames_to_patches(frames: Tensor, frame_index: Tensor, ref_rotations: Tensor,
                      ref_translations: Tensor, ori_k: Tensor, labels: Tensor, points: Tensor,
                      counts: Tensor, size: int = 256, size_ratio: Union[float, Tensor] = 1.1,
                      pad_val: float = 128, img_norm_cfg: Optional[dict] = None,
                      to_rgb: bool = True) -> Dict[str, Tensor]:
    """Decoded frames [F, H, W, 3] uint8 (interleaved, as cv2 decodes them) plus N detections —
    frame_index [N], reference poses [N, 3, 3] / [N, 3], labels [N], intrinsics ori_k [N, 3, 3] or
    one per frame [F, 3, 3] — to what ``format_data_test`` hands the refiner:

    * ``real_images`` [N, 3, size, size] float32, normalised with ``img_norm_cfg`` (``mean`` /
      ``std`` in output channel order, mmcv ``imnormalize``; default the config's 0 / 255) after
      ``to_rgb`` reversed the channels;
    * ``internel_k`` [N, 3, 3] = ``transform_matrix`` · ``ori_k``, ``transform_matrix`` [N, 3, 3],
      ``ori_k`` [N, 3, 3] (per object);
    * ``valid`` [N] bool and ``crop_boxes`` [N, 4] int32 (x1, y1, x2, y2, inclusive); also the raw
      ``geom`` [N, 8] int32 for ``extract_maps`` and ``bboxes`` [N, 4].

    ``points`` / ``counts``: the model point table (``point_table``).  ``size_ratio``: the crop's
    side over the box's, 1.1 at test time; a tensor [N] gives every object its own — the training
    pipeline's ``U(1.0, 1.25)``, which ``frames_to_train_patches`` draws on the device.  An invalid
    object (behind the camera, off the frame, …) gets a ``pad_val`` patch, the identity transform
    and ``internel_k = ori_k``.
    Everything runs on the current stream without a host synchronisation."""
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
        raise ScflowError("frames must be a [F, H, W, 3] uint8 tensor")
    f, h, w, _ = frames.shape
    n = labels.shape[0]
    cfg = dict(IMG_NORM_CFG if img_norm_cfg is None else img_norm_cfg)
    to_rgb = bool(cfg.get("to_rgb", to_rgb))
    fidx = _i32(frame_index)
    per_frame = ori_k.shape[0] != n
    if per_frame and ori_k.shape[0] != f:
        raise ScflowError(f"ori_k must be [{n}, 3, 3] or [{f}, 3, 3], got {list(ori_k.shape)}")
    if isinstance(size_ratio, torch.Tensor):
        ratio = size_ratio.contiguous().float()
    else:
        ratio = torch.full((n,), float(size_ratio), device=frames.device, dtype=torch.float32)
    ori_k = ori_k.contiguous().float()
    bbox, geom, T, k, valid = ops.patch_boxes(
        points.contiguous().float(), _i32(counts), _i32(labels), ref_rotations.contiguous().float(),
        ref_translations.contiguous().float(), ori_k, ratio, h, w, size, frame_index=fidx,
        num_frames=f, k_per_frame=per_frame)
    images = ops.extract_patches(frames.contiguous(), fidx, geom, valid, size, pad=float(pad_val),
                                 mean=cfg["mean"], std=cfg["std"], to_rgb=to_rgb)
    if per_frame:  # an index outside the frames made its object invalid; clamp it for the gather
        ori_k = ori_k[fidx.clamp(0, f - 1).long()]
    return dict(real_images=images, internel_k=k, transform_matrix=T, ori_k=ori_k,
                valid=valid != 0, crop_boxes=geom[:, :4], geom=geom, bboxes=bbox)


def extract_maps(maps: Tensor, frame_index: Tensor, geom: Tensor, valid: Optional[Tensor] = None,
                 size: int = 256, mode: str = "bilinear") -> Tensor:
    """Single-channel maps [F, H, W] or [F, H, W, 1] (float32 depth, uint8 masks) under the
    geometry ``frames_to_patches`` returned (``geom`` [N, 8], ``valid`` [N] bool / uint8 or None =
    all valid) → [N, 1, size, size] float32.  ``mode='bilinear'`` (depth): cv2's INTER_LINEAR, pad
    0, not quantised; ``mode='nearest'`` (masks): the nearest source pixel, pad 0.

    The result is DEFINED by ``transform_matrix``: pixel (u, v) of a map patch shows the frame
    point T⁻¹(u, v), as the image patch does.  The reference's ``BitmapMasks.crop / rescale / pad``
    are not reproduced: they take the crop box as exclusive (one column and row fewer than mmcv's
    inclusive ``imcrop`` of the image), so its masks land up to a pixel off its own image."""
    if mode not in ("bilinear", "nearest"):
        raise ScflowError(f"extract_maps: mode must be 'bilinear' or 'nearest', got {mode!r}")
    if isinstance(maps, torch.Tensor) and maps.dim() == 3:
        maps = maps.unsqueeze(-1)
    n = geom.shape[0]
    if valid is None:
        valid = torch.ones(n, device=geom.device, dtype=torch.uint8)
    return ops.extract_patches(maps.contiguous(), _i32(frame_index), geom.contiguous(),
                               valid.contiguous().to(torch.uint8), size, pad=0.0, quantize=False,
                               nearest=mode == "nearest")


# ------------------------------------------------------------------------------ training
# configs/refine_models/scflow_ycbv_real.py:53-75: PoseJitter, Crop(size_range), RandomHSV,
# RandomNoise, RandomSmooth (each colour transform with its default p = 1).  A limit below 0 is
# off; a stage with p < 0 never runs.
TRAIN_AUG = dict(angle_mean=0.0, angle_std=15.0, x_mean=0.0, y_mean=0.0, z_mean=0.0, x_std=15.0,
                 y_std=15.0, z_std=50.0, angle_limit=45.0, translation_limit=200.0, add_limit=1.0,
                 ratio_lo=1.0, ratio_hi=1.25, h_ratio=0.2, s_ratio=0.5, v_ratio=0.5,
                 noise_ratio=0.1, max_kernel_size=5, p_hsv=1.0, p_noise=1.0, p_blur=1.0)


def frames_to_train_patches(frames: Tensor, masks: Tensor, frame_index: Tensor,
                            gt_rotations: Tensor, gt_translations: Tensor, ori_k: Tensor,
                            labels: Tensor, points: Tensor, counts: Tensor, diameters: Tensor,
                            seed: int, step: int, aug: Optional[dict] = None, size: int = 256,
                            object_offset: int = 0, max_tries: int = 32, pad_val: int = 128,
                            img_norm_cfg: Optional[dict] = None, to_rgb: bool = True, *,
                            backgrounds: Optional[Tensor] = None,
                            background_sizes: Optional[Tensor] = None, background_p: float = 0.3,
                            background_index: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """Decoded frames [F, H, W, 3] uint8 (BGR) and their instance masks [F, H, W] uint8 plus N
    annotated objects — frame_index [N], GT poses, labels, ori_k per object or per frame — to the
    real-image half of a training batch, as the reference's training pipeline formats it
    (configs/refine_models/scflow_ycbv_real.py:50-93) but in four launches for all objects:
    ``ops.train_draw`` (jittered pose, crop ratio, colour parameters), ``ops.patch_boxes`` at the
    jittered pose with the drawn ratio, ``ops.extract_patches_aug`` and ``extract_maps`` of the
    masks (nearest).  ``aug``: ``TRAIN_AUG`` with any key replaced; ``diameters`` [C] float32.

    Returns ``real_images`` [N, 3, size, size], ``gt_masks`` [N, size, size] (0 / 1),
    ``internel_k``, ``transform_matrix``, ``ref_rotation`` / ``ref_translation`` (jittered),
    ``gt_rotation`` / ``gt_translation``, ``label`` (int64), ``valid`` [N] bool (the crop is one
    AND a jitter try was accepted), ``init_add_error`` / ``init_rot_error`` / ``init_trans_error``
    [N], ``tries``, ``ratio``, ``aug`` [N, 8] and ``geom`` [N, 8].  Every random number is a
    function of (seed, step, object_offset + i): a data-parallel rank passes the
    number of objects before its own as ``object_offset``.  An invalid object gets a ``pad_val``
    patch.  Everything runs on the current stream without a host synchronisation.

    ``backgrounds`` [B, Hb, Wb, 3] uint8 BGR adds the reference's ``RandomBackground(p=
    background_p)`` between the crop and the colour stages (configs/refine_datasets/
    ycbv_mixpbr.py:49) in the same launch (``ops.extract_patches_aug_bg`` with
    ``masks`` as the foreground): ``background_sizes`` [B, 2] int32 gives the used (height, width)
    of each slot, ``background_index`` [N] replaces the draw (−1: none), and the result gains
    ``background_index`` [N] int32, the slot every object got (−1: none).  Loading a directory of
    images into the pool is the caller's."""
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
        raise ScflowError("frames must be a [F, H, W, 3] uint8 tensor")
    f, h, w, _ = frames.shape
    n = labels.shape[0]
    cfg = dict(TRAIN_AUG)
    cfg.update(aug or {})
    norm = dict(IMG_NORM_CFG if img_norm_cfg is None else img_norm_cfg)
    to_rgb = bool(norm.get("to_rgb", to_rgb))
    fidx, lab = _i32(frame_index), _i32(labels)
    per_frame = ori_k.shape[0] != n
    if per_frame and ori_k.shape[0] != f:
        raise ScflowError(f"ori_k must be [{n}, 3, 3] or [{f}, 3, 3], got {list(ori_k.shape)}")
    points, counts = points.contiguous().float(), _i32(counts)
    R_gt, t_gt = gt_rotations.contiguous().float(), gt_translations.contiguous().float()
    R, t, err, ok, tries, ratio, rows = ops.train_draw(
        points, counts, lab, diameters.contiguous().float(), R_gt, t_gt, cfg, seed, step,
        object_offset, max_tries)
    _, geom, T, k, valid = ops.patch_boxes(points, counts, lab, R, t, ori_k.contiguous().float(),
                                           ratio, h, w, size, frame_index=fidx, num_frames=f,
                                           k_per_frame=per_frame)
    extra = {}
    if backgrounds is None:
        images = ops.extract_patches_aug(frames.contiguous(), fidx, geom, valid, rows, size, seed,
                                         step, object_offset, pad=pad_val, mean=norm["mean"],
                                         std=norm["std"], to_rgb=to_rgb)
    else:
        flat = masks[..., 0] if isinstance(masks, torch.Tensor) and masks.dim() == 4 else masks
        index = None if background_index is None else _i32(background_index)
        images, extra["background_index"] = ops.extract_patches_aug_bg(
            frames.contiguous(), flat.contiguous(), fidx, geom, valid, rows, backgrounds, size,
            seed, step, object_offset, p=background_p, background_sizes=background_sizes,
            background_index=index, pad=pad_val, mean=norm["mean"], std=norm["std"], to_rgb=to_rgb)
    gt_masks = extract_maps(masks, fidx, geom, valid, size, mode="nearest")[:, 0]
    return dict(extra, real_images=images, gt_masks=(gt_masks > 0).float(), internel_k=k,
                transform_matrix=T, ref_rotation=R, ref_translation=t, gt_rotation=R_gt,
                gt_translation=t_gt, label=labels.long(), valid=(valid != 0) & (ok != 0),
                init_add_error=err[:, 0], init_rot_error=err[:, 1], init_trans_error=err[:, 2],
                tries=tries, ratio=ratio, aug=rows, geom=geom)
