"""BOP pose errors and average recall (bop_toolkit's ``pose_error.py`` / ``misc.py`` with the
BOP19 settings), the metric behind SCFlow's published YCB-V numbers.  The reference dumps BOP
results (``bop_eval.format_results``) and leaves the scoring to that CPU toolkit; here the three
error functions run on the device (include/scflow_hip.h: ``scflow_pose_err_sym``,
``scflow_vsd_counts``) and only the thresholding runs on the host.  DESIGN.md §22 has the
definitions and what stays unpinned: the toolkit itself is absent, so parity with its renderer's
depth at silhouette edges, its symmetry enumeration and its greedy matching is not tested.

* ``symmetry_transforms`` / ``symmetry_table`` — the symmetry set of a ``models_info.json`` entry:
  identity + discrete symmetries, times each continuous symmetry discretised into
  ``ceil(π / max_sym_disc_step)`` rotations.
* ``mssd_mspd`` — maximum symmetry-aware surface / projection distance, one launch.
* ``vsd_counts`` / ``vsd`` — visible surface discrepancy ('bop19' visibility, step cost) from depth
  renders of the existing ``Renderer``.
* ``recall`` / ``average_recall`` — BOP19 average recall on the host in float64.
"""
from __future__ import annotations

import math
from typing import Dict, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import ScflowError

Tensor = torch.Tensor

BOP19_TAUS = tuple(round(0.05 * k, 2) for k in range(1, 11))       # VSD misalignment tolerances
BOP19_THETAS = tuple(round(0.05 * k, 2) for k in range(1, 11))     # VSD / MSSD (·diameter) thresholds
BOP19_MSPD_THETAS = tuple(5.0 * k for k in range(1, 11))           # px at a 640-wide frame
BOP19_DELTA = 15.0                                                 # mm
MAX_SYM_DISC_STEP = 0.01


# ------------------------------------------------------------------------------ symmetry sets
def _axis_rotation(axis: np.ndarray, angle: float) -> np.ndarray:
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * k + (1.0 - math.cos(angle)) * (k @ k)


def symmetry_transforms(model_info: Optional[Mapping], max_sym_disc_step: float = MAX_SYM_DISC_STEP
                        ) -> np.ndarray:
    """[S, 3, 4] float64 [R | t] of one ``models_info.json`` entry (None: the identity alone).

    ``disc`` = identity + every ``symmetries_discrete`` entry (16 floats, a row-major 4×4).  Each
    ``symmetries_continuous`` ``{axis, offset}`` gives ``count = ceil(π / max_sym_disc_step)``
    rotations by i·2π/count, i = 0 … count−1, about the normalised axis through ``offset``
    (t = −R·offset + offset).  The set is every product cont∘disc (R = R_c·R_d, t = R_c·t_d + t_c);
    without a continuous symmetry, ``disc`` alone.  i = 0 is included so that the set always holds
    the identity: the project's definition (parity with the toolkit's enumeration is unpinned)."""
    info = model_info or {}
    disc = [np.hstack([np.eye(3), np.zeros((3, 1))])]
    for s in info.get("symmetries_discrete", ()):
        m = np.asarray(s, np.float64).reshape(4, 4)
        disc.append(m[:3, :4].copy())
    conts = []
    for c in info.get("symmetries_continuous", ()):
        count = int(math.ceil(math.pi / max_sym_disc_step))
        off = np.asarray(c.get("offset", (0.0, 0.0, 0.0)), np.float64).reshape(3)
        for i in range(count):
            R = _axis_rotation(c["axis"], i * 2.0 * math.pi / count)
            conts.append((R, -R @ off + off))
    if not conts:
        return np.stack(disc)
    out = []
    for Rc, tc in conts:
        for d in disc:
            out.append(np.hstack([Rc @ d[:, :3], (Rc @ d[:, 3] + tc)[:, None]]))
    return np.stack(out)


def symmetry_table(models_info: Mapping, num_classes: int, device="cuda",
                   max_sym_disc_step: float = MAX_SYM_DISC_STEP) -> Tuple[Tensor, Tensor]:
    """(table [T, 12] float32, offsets [num_classes + 1] int32) on ``device``: class ``l`` (the
    0-based label; BOP obj_id l + 1, looked up as ``l + 1`` or ``str(l + 1)``) owns rows
    ``offsets[l] : offsets[l + 1]``, each a row-major 3×4.  A class without an entry gets the
    identity alone."""
    rows, off = [], [0]
    for lab in range(num_classes):
        info = models_info.get(str(lab + 1), models_info.get(lab + 1))
        t = symmetry_transforms(info, max_sym_disc_step)
        rows.append(t.reshape(-1, 12))
        off.append(off[-1] + t.shape[0])
    table = torch.from_numpy(np.concatenate(rows).astype(np.float32)).to(device)
    return table, torch.tensor(off, dtype=torch.int32).to(device)


# ------------------------------------------------------------------------------ device errors
def _f32(x: Tensor) -> Tensor:
    return x.to(torch.float32).contiguous()


def _i32(x: Tensor) -> Tensor:
    return x.to(torch.int32).contiguous()


def mssd_mspd(points: Tensor, counts: Tensor, sym_table: Tensor, sym_offset: Tensor, labels: Tensor,
              R_est: Tensor, t_est: Tensor, R_gt: Tensor, t_gt: Tensor, K: Optional[Tensor] = None,
              which: str = "both") -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """(mssd [N] in model units, mspd [N] in px) of N (estimate, ground truth) pairs:

        MSSD = min_{S ∈ Sym} max_{x ∈ V} ‖(R̂x + t̂) − (R̄(S_R x + S_t) + t̄)‖₂
        MSPD = the same with both points projected by K ((K·X)[:2] / (K·X)[2])

    over the vertices ``points[l, :counts[l]]`` (``patches.point_table``) and the symmetry set of
    the estimate's class (``symmetry_table``); +inf for a class without vertices.  One launch, no
    [N, S, P] intermediate, no host synchronisation; bitwise reproducible.  ``which``: 'both'
    ('mssd' when K is None), 'mssd' or 'mspd' — the one not computed is None."""
    if which not in ("both", "mssd", "mspd"):
        raise ValueError(f"which = {which!r}")
    want_s = which in ("both", "mssd")
    want_p = which == "mspd" or (which == "both" and K is not None)
    if want_p and K is None:
        raise ScflowError("mspd needs K")
    return ops.pose_err_sym(_f32(points), _i32(counts), _f32(sym_table), _i32(sym_offset), _i32(labels),
                            _f32(R_est), _f32(t_est), _f32(R_gt), _f32(t_gt),
                            None if K is None else _f32(K), want_s, want_p)


def vsd_counts(depth_est: Tensor, depth_gt: Tensor, depth_test: Tensor, frame_index: Tensor, K: Tensor,
               diameters: Optional[Tensor], taus: Sequence[float] = BOP19_TAUS,
               delta: float = BOP19_DELTA) -> Tensor:
    """[N, 2 + n_taus] int32 (|U|, |I|, cost_k …) of N pairs (``scflow_vsd_counts``): depth_est /
    depth_gt [N, H, W] (≤ 0 empty), depth_test [F, H, W] (0: no measurement) read at
    ``frame_index``, ``diameters`` [N] or None (costs not normalised).  Exact integers."""
    dev = depth_est.device
    t = taus if isinstance(taus, torch.Tensor) else torch.tensor(list(taus), dtype=torch.float32)
    return ops.vsd_counts(_f32(depth_est), _f32(depth_gt), _f32(depth_test), _i32(frame_index), _f32(K),
                          None if diameters is None else _f32(diameters), _f32(t.to(dev)), delta)


def vsd_errors(counts: Tensor) -> Tensor:
    """[N, n_taus] float64: e_k = (cost_k + |U| − |I|) / |U|, and 1 where |U| = 0."""
    c = counts.to(torch.float64)
    u, i = c[:, :1], c[:, 1:2]
    return torch.where(u > 0, (c[:, 2:] + u - i) / u.clamp(min=1.0), torch.ones_like(c[:, 2:]))


def vsd(renderer, labels: Tensor, R_est: Tensor, t_est: Tensor, R_gt: Tensor, t_gt: Tensor, K: Tensor,
        depth_test: Tensor, frame_index: Tensor, diameters: Tensor,
        taus: Sequence[float] = BOP19_TAUS, delta: float = BOP19_DELTA) -> Tensor:
    """Visible surface discrepancy [N, n_taus] float64 (on the device) of N pairs against the
    sensor depth ``depth_test`` [F, H, W] of their frames.  Both pose sets are rendered on
    ``renderer`` (only ``fragments.zbuf`` is used) with the frame's own K; the renderer is square,
    so it must be at least max(H, W) wide and rows [:H], columns [:W] of its render are the frame
    (K is in pixels: pixel (x, y) of the render is the frame's pixel (x, y))."""
    _, h, w = depth_test.shape
    s = renderer.image_size[0]
    if s < max(h, w):
        raise ScflowError(f"vsd: the renderer is {s}² and the frame {h}×{w}: build a Renderer with "
                          f"image_size ≥ {max(h, w)}")
    lab = labels.to(torch.long)
    z_est = renderer(R_est, t_est, K, lab)["fragments"].zbuf[:, :h, :w, 0]
    z_gt = renderer(R_gt, t_gt, K, lab)["fragments"].zbuf[:, :h, :w, 0]
    return vsd_errors(vsd_counts(z_est, z_gt, depth_test, frame_index, K, diameters, taus, delta))


def vsd_frames(table, labels: Tensor, R_est: Tensor, t_est: Tensor, R_gt: Tensor, t_gt: Tensor, K: Tensor,
               depth_test: Tensor, frame_index: Tensor, diameters: Tensor,
               taus: Sequence[float] = BOP19_TAUS, delta: float = BOP19_DELTA) -> Tensor:
    """``vsd`` without the square renderer: both pose sets are rendered at the frames' own H × W
    by ``scene.scene_visibility`` (``want=("depth_inst",)``, two calls) from a ``scene.mesh_table``
    and go to ``vsd_counts`` / ``vsd_errors``.  K [N, 3, 3] per pair, as for ``vsd`` (the pairs of
    one frame share it).  The pixel convention is scene visibility's (integer
    coordinates are pixel centres), not the square renderer's: the two functions' depth maps differ
    along silhouettes."""
    from . import scene
    f, h, w = depth_test.shape
    fi = frame_index.to(torch.int64)
    # per-frame K from the pairs' (a frame_index outside the frames lands in a row that is dropped)
    row = torch.where((fi >= 0) & (fi < f), fi, torch.full_like(fi, f))
    kf = torch.zeros(f + 1, 3, 3, dtype=torch.float32, device=K.device).index_copy_(0, row, _f32(K))[:f]
    z_est = scene.scene_visibility(table, labels, fi, R_est, t_est, kf, h, w, want=("depth_inst",))["depth_inst"]
    z_gt = scene.scene_visibility(table, labels, fi, R_gt, t_gt, kf, h, w, want=("depth_inst",))["depth_inst"]
    return vsd_errors(vsd_counts(z_est, z_gt, depth_test, frame_index, K, diameters, taus, delta))


# ------------------------------------------------------------------------------ recall (host)
def recall(errors, thresholds, targets) -> np.ndarray:
    """Recall per threshold, float64: the number of target instances whose error is below the
    threshold (strictly) over the number of targets (0 when there is none).  ``errors`` [M] or
    [M, A] (+inf: a GT without a matched estimate, never correct); ``thresholds`` [T], or [M, T]
    when they scale per instance; ``targets`` [M] bool.  → [T], or [A, T]."""
    e = np.asarray(errors, np.float64)
    th = np.asarray(thresholds, np.float64)
    tg = np.asarray(targets, bool)
    if th.ndim == 1:
        th = np.broadcast_to(th[None], (e.shape[0], th.shape[0]))
    n = int(tg.sum())
    if e.ndim == 1:
        ok = e[:, None] < th
        return ok[tg].sum(0) / n if n else np.zeros(th.shape[1])
    ok = e[:, :, None] < th[:, None, :]
    return ok[tg].sum(0) / n if n else np.zeros((e.shape[1], th.shape[1]))


def average_recall(vsd_e, mssd_e, mspd_e, diameters, width: int, targets) -> Dict[str, object]:
    """BOP19 average recall.  ``vsd_e`` [M, 10] (one column per τ), ``mssd_e`` / ``mspd_e`` [M],
    ``diameters`` [M] per GT instance, ``width`` of the frames, ``targets`` [M] bool (the GT
    instances that count: ``visib_fract`` ≥ 0.1).  An estimate is correct when its error is below
    θ: VSD θ ∈ {0.05 … 0.5} for every τ; MSSD θ·diameter; MSPD θ ∈ {5 … 50}·width/640 px.
    → AR_VSD / AR_MSSD / AR_MSPD (the mean recall over the thresholds), AR (their mean) and the
    per-threshold recalls ``recall_vsd`` [τ, θ], ``recall_mssd`` [θ], ``recall_mspd`` [θ]."""
    d = np.asarray(diameters, np.float64)
    th = np.asarray(BOP19_THETAS, np.float64)
    r_vsd = recall(vsd_e, th, targets)
    r_mssd = recall(mssd_e, th[None, :] * d[:, None], targets)
    r_mspd = recall(mspd_e, np.asarray(BOP19_MSPD_THETAS, np.float64) * (float(width) / 640.0), targets)
    out = {"AR_VSD": float(r_vsd.mean()), "AR_MSSD": float(r_mssd.mean()), "AR_MSPD": float(r_mspd.mean())}
    out["AR"] = (out["AR_VSD"] + out["AR_MSSD"] + out["AR_MSPD"]) / 3.0
    out.update(recall_vsd=r_vsd, recall_mssd=r_mssd, recall_mspd=r_mspd)
    return out
