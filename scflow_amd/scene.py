"""Scene visibility on the device: instance masks, ``visib_fract`` and boxes from posed meshes.

What a ready-made BOP data set ships as ``mask_visib`` PNGs and ``scene_gt_info.json`` (bop_toolkit's
``calc_gt_masks`` / ``calc_gt_info``: one CPU render per instance), computed here for all instances
of all frames of a batch in one call (include/scflow_hip.h: ``scflow_scene_visibility``; DESIGN.md
§23 has the definitions, which are the project's own — parity with the toolkit is unpinned).

* ``mesh_table`` — the classes' meshes packed once into device arrays (mirrors
  ``patches.point_table``): nothing is re-packed per call and labels are never read on the host.
* ``scene_visibility`` — the call, for instances in any frame order.
* ``visib_fract`` / ``foreground_masks`` — what ``bop_eval.evaluate_bop`` thresholds and what
  ``patches.frames_to_train_patches(masks=…)`` takes.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Mapping, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops
from ._lib import ScflowError

Tensor = torch.Tensor

STAT_COLUMNS = ("px_count_all", "px_count_valid", "px_count_visib")   # stats[:, 0:3]
BBOX_OBJ, BBOX_VISIB = slice(3, 7), slice(7, 11)                      # (x, y, w, h) each


@dataclass
class MeshTable:
    """Class ``l`` owns ``verts[vert_offset[l]:vert_offset[l+1]]`` and
    ``faces[face_offset[l]:face_offset[l+1]]`` (vertex indices local to that block); ``bounds[l]``
    = (min x, y, z, max x, y, z) of its vertices.  A class without a mesh has empty ranges."""
    verts: Tensor        # [ΣV, 3] float32
    faces: Tensor        # [ΣF, 3] int32
    vert_offset: Tensor  # [C + 1] int32
    face_offset: Tensor  # [C + 1] int32
    bounds: Tensor       # [C, 6] float32

    @property
    def num_classes(self) -> int:
        return self.bounds.shape[0]


def mesh_table(renderer_or_meshes, device=None) -> MeshTable:
    """The meshes of a ``Renderer`` (its ``meshes`` {label: (verts, faces, …)}) or such a mapping
    itself (tensors or arrays) as one ``MeshTable`` on ``device`` (default: the meshes' own)."""
    meshes: Mapping = getattr(renderer_or_meshes, "meshes", renderer_or_meshes)
    if not meshes:
        raise ScflowError("mesh_table: no mesh")
    c = max(int(l) for l in meshes) + 1
    vs, fs, voff, foff = [], [], [0], [0]
    bounds = np.zeros((c, 6), np.float32)
    by_label = {int(l): m for l, m in meshes.items()}
    for lab in range(c):
        if lab in by_label:
            v, f = by_label[lab][0], by_label[lab][1]
            if device is None and isinstance(v, torch.Tensor):
                device = v.device
            v = torch.as_tensor(np.array(v.cpu() if isinstance(v, torch.Tensor) else v)).to(torch.float32)
            f = torch.as_tensor(np.array(f.cpu() if isinstance(f, torch.Tensor) else f)).to(torch.int32)
            v, f = v.reshape(-1, 3), f.reshape(-1, 3)
            if v.shape[0] and f.shape[0]:
                vs.append(v)
                fs.append(f)
                bounds[lab, :3] = v.min(0).values.numpy()
                bounds[lab, 3:] = v.max(0).values.numpy()
        voff.append(sum(x.shape[0] for x in vs))
        foff.append(sum(x.shape[0] for x in fs))
    if not vs:
        raise ScflowError("mesh_table: every mesh is empty")
    dev = torch.device("cpu" if device is None else device)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32).to(dev)  # noqa: E731
    return MeshTable(torch.cat(vs).contiguous().to(dev), torch.cat(fs).contiguous().to(dev), i32(voff),
                     i32(foff), torch.from_numpy(bounds).to(dev))


def scene_visibility(table: MeshTable, labels: Tensor, frame_index: Tensor, R: Tensor, t: Tensor,
                     K: Tensor, height: int, width: int, depth_test: Union[Tensor, None] = None,
                     delta: float = 15.0, margin: Tuple[int, int] = (0, 0), pixel_offset: float = 0.0,
                     want: Sequence[str] = ("stats", "inst_id")) -> Dict[str, Tensor]:
    """Which instance is seen where, and how much of each, for n posed instances in F frames of
    ``height`` × ``width``: labels / frame_index [n] (any order), R [n, 3, 3], t [n, 3], K
    [F, 3, 3], ``depth_test`` [F, H, W] sensor depth in mm (0: no measurement) or None (mutual
    occlusion only), ``margin`` = (x, y) pixels of canvas around the frame for ``px_count_all`` and
    ``bbox_obj``.  Returns the tensors named in ``want``:

    * ``stats`` [n, 12] int32: px_count_all, px_count_valid, px_count_visib, bbox_obj (x, y, w, h),
      bbox_visib (x, y, w, h), 0; an empty box is (−1, −1, −1, −1);
    * ``inst_id`` [F, H, W] int32: the index (in the caller's order) of the nearest visible
      instance, −1 if none;
    * ``depth_scene`` [F, H, W]: the nearest depth over the frame's instances, 0 if none;
    * ``depth_inst`` [n, H, W] (0 where empty) and ``mask_visib`` [n, H, W] uint8 per instance.

    The instances are sorted by frame with a stable argsort on the device, and the per-instance
    outputs and ``inst_id`` are mapped back to the caller's order; no host synchronisation."""
    fi = frame_index.to(torch.int64)
    order = torch.argsort(fi, stable=True)
    out = ops.scene_visibility(
        table.verts, table.faces, table.vert_offset, table.face_offset, table.bounds,
        labels.to(torch.int32)[order].contiguous(), fi[order].to(torch.int32).contiguous(),
        R.to(torch.float32)[order].contiguous(), t.to(torch.float32)[order].contiguous(),
        K.to(torch.float32).contiguous(), height, width,
        None if depth_test is None else depth_test.to(torch.float32).contiguous(), delta, margin,
        pixel_offset, want)
    res = {}
    for name, x in out.items():
        if name in ("stats", "depth_inst", "mask_visib"):
            res[name] = torch.empty_like(x).index_copy_(0, order, x)
        elif name == "inst_id" and order.numel():
            res[name] = torch.where(x >= 0, order[x.clamp(min=0).long()].to(torch.int32), x)
        else:
            res[name] = x
    return res


def visib_fract(stats: Tensor) -> Tensor:
    """[n] float64: px_count_visib / px_count_all, and 0 where px_count_all = 0."""
    s = stats.to(torch.float64)
    return torch.where(s[:, 0] > 0, s[:, 2] / s[:, 0].clamp(min=1.0), torch.zeros_like(s[:, 0]))


def foreground_masks(inst_id: Tensor) -> Tensor:
    """[F, H, W] uint8: 1 where any instance is visible — the ``masks`` of
    ``patches.frames_to_train_patches`` and ``SCFlowRefiner.train_batch_from_frames``."""
    return (inst_id >= 0).to(torch.uint8)
