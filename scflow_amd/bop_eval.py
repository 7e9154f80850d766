"""BOP-format pose evaluation: the host side of the reference's ``ADD``
metric (metrics/add.py) around the numeric core in ``metrics.py``.

* ``load_bop_annotations`` — per sequence ``scene_gt.json`` / ``scene_camera.json`` /
  ``scene_gt_info.json`` (add.py:71-89 ``_load_pose_annots``; the BOP layout ``{seq:06d}/…``).
* ``match_results`` — prediction ↔ GT matching (add.py:184-255): for every GT object of an
  image, the one prediction of its class, or — several predictions of that class — the one with
  the smallest normalised ADD(-S), or none (invalid; errors filled with the reference's 1 / 50 px
  / 110 values, add.py:158-160).
* ``parse_error_to_metric`` — class-wise precision at the thresholds (add.py:261-330: per class
  the fraction with error < thr, −1 for an absent class, the average over present classes per
  threshold) and the ``{class}/{metric}`` dictionary of ``parse_metric_to_tensorboard``.
* ``evaluate`` — compute_metrics (add.py:134-180): match, ADD(-S)/diameter + reprojection error
  (``metrics.pose_errors``), the table.
* ``format_results`` — predictions dumped as BOP ``scene_gt.json`` per sequence (add.py:402-446).
* ``load_models_info`` / ``load_depth`` / ``evaluate_bop`` — BOP19 average recall over VSD, MSSD
  and MSPD (``bop_metrics``), what the reference leaves to bop_toolkit after ``format_results``.

Inputs are plain dicts / arrays (the reference's ``results`` entries: ``img_metas.img_path``,
``pred.labels / rotations / translations``); model points are passed in (the reference samples
1000 mesh vertices at random per class with trimesh — once in match_results, add.py:190, and
again in compute_metrics, add.py:157 — trimesh and the meshes are absent here, so the caller
supplies both point sets).  Parity: pinned by ``tests/golden/golden_metric_add.npz``, generated
from the reference's own ``ADD`` class (constructed with its real ``__init__`` on a synthetic BOP
tree, ``make_golden.py metric``) — compute_metrics end to end, match_results, eval_pose_error,
parse_error_to_metric and the scene_gt.json text (tests/test_metric_golden.py).
"""
from __future__ import annotations

import json
import os
import os.path as osp
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .metrics import pose_errors

POSE_JSON = "{:06d}/scene_gt.json"
INFO_JSON = "{:06d}/scene_gt_info.json"
CAMERA_JSON = "{:06d}/scene_camera.json"


def load_bop_annotations(annots_root: str, sequences: Sequence[str]) -> Dict[str, dict]:
    """{sequence: {'pose': scene_gt, 'camera': scene_camera, 'gt_info': scene_gt_info (if any)}}."""
    out = {}
    for seq in sequences:
        sid = int(seq)
        d = {}
        for key, tmpl in (("pose", POSE_JSON), ("camera", CAMERA_JSON), ("gt_info", INFO_JSON)):
            path = osp.join(annots_root, tmpl.format(sid))
            if osp.exists(path):
                with open(path) as f:
                    d[key] = json.load(f)
        out[seq] = d
    return out


def _seq_and_image(img_path: str) -> Tuple[str, int]:
    """add.py:193-198: '…/{seq}/rgb/{img}.png' → (seq, image id)."""
    parts = img_path.rsplit("/", 3)
    seq, img_name = (parts[0], parts[2]) if len(parts) == 3 else (parts[1], parts[3])
    return seq, int(osp.splitext(img_name)[0])


def _errors(points, gt_r, gt_t, pred_r, pred_t, labels0, k, symmetric, diameters):
    """metrics.pose_errors on float64 CPU tensors → numpy (add, rep, add_mm)."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)  # noqa: E731
    e = pose_errors([t(p) for p in points], t(gt_r), t(gt_t), t(pred_r), t(pred_t),
                    torch.as_tensor(np.asarray(labels0), dtype=torch.int64), t(k), symmetric, diameters)
    return e["add"].numpy(), e["rep"].numpy(), e["add_mm"].numpy()


def match_results(results: Sequence[dict], gt_annots: Dict[str, dict], points: Sequence[np.ndarray],
                  symmetric: Sequence[int], diameters: Sequence[float],
                  inverse_label_mapping: Optional[Dict[int, int]] = None):
    """(gt_R [M,3,3], gt_t [M,3], pred_R, pred_t, labels0 [M] (0-based), valid [M] bool, K [M,3,3])
    over every GT object of every result's image (add.py:184-255)."""
    inv = inverse_label_mapping or {}
    gR, gT, pR, pT, K, valid, labels = [], [], [], [], [], [], []
    for res in results:
        seq, img_id = _seq_and_image(res["img_metas"]["img_path"])
        ann = gt_annots[seq]
        gt_objs = ann["pose"][str(img_id)]
        k = np.asarray(ann["camera"][str(img_id)]["cam_K"], dtype=np.float32).reshape(3, 3)
        pred = res["pred"]
        pl = np.array([inv.get(int(l) + 1, int(l) + 1) for l in np.asarray(pred["labels"])], dtype=np.int64)
        prs = np.asarray(pred["rotations"], dtype=np.float32).reshape(-1, 3, 3)
        pts = np.asarray(pred["translations"], dtype=np.float32).reshape(-1, 3)
        for obj in gt_objs:
            oid = int(obj["obj_id"])
            R = np.asarray(obj["cam_R_m2c"], dtype=np.float32).reshape(3, 3)
            tt = np.asarray(obj["cam_t_m2c"], dtype=np.float32).reshape(-1)
            gR.append(R)
            gT.append(tt)
            K.append(k)
            labels.append(oid)
            m = pl == oid
            nm = int(m.sum())
            if nm == 1:
                j = int(np.nonzero(m)[0][0])
                pR.append(prs[j])
                pT.append(pts[j])
                valid.append(True)
            elif nm > 1:  # the candidate with the smallest normalised ADD(-S)
                add, _, _ = _errors(points, np.repeat(R[None], nm, 0), np.repeat(tt[None], nm, 0),
                                    prs[m], pts[m], np.full(nm, oid - 1), np.repeat(k[None], nm, 0),
                                    symmetric, diameters)
                full = np.full(m.shape[0], 100.0, dtype=np.float32)
                full[m] = add
                j = int(np.argmin(full))
                pR.append(prs[j])
                pT.append(pts[j])
                valid.append(True)
            else:
                pR.append(np.zeros((3, 3), np.float32))
                pT.append(np.zeros(3, np.float32))
                valid.append(False)
    return (np.stack(gR), np.stack(gT), np.stack(pR), np.stack(pT),
            np.asarray(labels, np.int64) - 1, np.asarray(valid, bool), np.stack(K))


def parse_error_to_metric(error_dict: Dict[str, np.ndarray], labels: np.ndarray,
                          metrics: Dict[str, Sequence[float]], class_names: Sequence[str]):
    """(metric_dict {'average': [...], class: [...]}, headers) as add.py:261-330 for the
    thresholded metrics ('add', 'rep'); metrics outside those two are skipped, as there."""
    metric_dict: Dict[str, List[float]] = {"average": []}
    headers = ["class"]
    per_class = {c: [] for c in class_names}
    avg_total: List[List[float]] = []
    for metric, thresholds in metrics.items():
        if metric not in ("add", "rep"):
            continue
        err = error_dict[metric]
        thresholds = list(thresholds)
        if not thresholds:  # already a per-sample quantity: class means
            headers.append(metric)
            for l, name in enumerate(class_names):
                sel = err[labels == l]
                per_class[name].append(-1 if sel.size == 0 else float(sel.mean()))
            avg_total.append(err.tolist())
            continue
        for thr in thresholds:
            headers.append("{}_{:0>2d}".format(metric, int(thr * 100)) if thr < 1
                           else "{}_{:0>2d}".format(metric, thr))
        avg = [[] for _ in thresholds]
        for l, name in enumerate(class_names):
            sel = err[labels == l]
            if sel.shape[0] == 0:
                per_class[name].extend([-1.0] * len(thresholds))
                continue
            for i, thr in enumerate(thresholds):
                v = float((sel < thr).sum() / sel.shape[0])
                per_class[name].append(v)
                avg[i].append(v)
        avg_total.extend(avg)
    metric_dict.update(per_class)
    metric_dict["average"] = [sum(p) / len(p) for p in avg_total]
    return metric_dict, headers


def to_flat_dict(metric_dict: Dict[str, List[float]], headers: Sequence[str]) -> Dict[str, float]:
    """parse_metric_to_tensorboard (add.py:344-351): {'{class}/{metric}': value}."""
    out = {}
    for name, vals in metric_dict.items():
        for i, h in enumerate(headers):
            if h != "class":
                out[f"{name}/{h}"] = vals[i - 1]
    return out


def evaluate(results: Sequence[dict], gt_annots: Dict[str, dict], points: Sequence[np.ndarray],
             class_names: Sequence[str], symmetric: Sequence[int], diameters: Sequence[float],
             metrics: Optional[Dict[str, Sequence[float]]] = None,
             inverse_label_mapping: Optional[Dict[int, int]] = None,
             match_points: Optional[Sequence[np.ndarray]] = None,
             round_digits: Optional[int] = 4) -> Dict[str, float]:
    """compute_metrics (add.py:134-180) → the flat '{class}/{metric}' dictionary.

    ``points``: the model points the errors are measured on (add.py:157); ``match_points``: those
    the duplicate-prediction matching uses (add.py:190; default ``points`` — the reference draws
    the two sets separately).  ``round_digits``: the reference's print_metric rounds every value
    to 4 decimals in place before parse_metric_to_tensorboard (add.py:334-339), so its returned
    dictionary holds rounded values; None keeps full precision."""
    metrics = metrics if metrics is not None else {"auc": [], "add": [0.05, 0.10, 0.20, 0.50]}
    gR, gT, pR, pT, labels, valid, K = match_results(
        results, gt_annots, points if match_points is None else match_points, symmetric, diameters,
        inverse_label_mapping)
    add = np.ones(labels.shape, np.float32)
    rep = np.full(labels.shape, 50.0, np.float32)
    if valid.any():
        a, r, _ = _errors(points, gR[valid], gT[valid], pR[valid], pT[valid], labels[valid], K[valid],
                          symmetric, diameters)
        add[valid] = a
        rep[valid] = r
    md, headers = parse_error_to_metric({"add": add, "rep": rep}, labels, metrics, class_names)
    if round_digits is not None:
        md = {k: [round(x, round_digits) for x in v] for k, v in md.items()}
    return to_flat_dict(md, headers)


def dumps_json(data, indent: int = 2, depth: int = 2) -> str:
    """JSON text as the reference's BOP dumps write it (datasets/utils.py:39-67): indented
    ``indent`` spaces per level, except that every container whose children would sit deeper
    than ``depth`` levels is written compactly on its opening line — for scene_gt.json, one line
    per predicted object."""
    def enc(v, level):
        if isinstance(v, (dict, list)) and v:
            if level >= depth:
                return json.dumps(v)
            pad = " " * (indent * (level + 1))
            end = "\n" + " " * (indent * level)
            if isinstance(v, dict):
                body = ",\n".join(f"{pad}{json.dumps(k)}: {enc(x, level + 1)}" for k, x in v.items())
                return "{\n" + body + end + "}"
            body = ",\n".join(pad + enc(x, level + 1) for x in v)
            return "[\n" + body + end + "]"
        return json.dumps(v)
    return enc(data, 0)


def format_results(results: Sequence[dict], data_root: str, save_dir: str,
                   inverse_label_mapping: Optional[Dict[int, int]] = None,
                   time: Optional[float] = None) -> List[str]:
    """Predictions written as BOP ``scene_gt.json`` per sequence under save_dir (add.py:402-446,
    the reference's dumps_json layout); returns the written paths."""
    inv = inverse_label_mapping or {}
    per_seq: Dict[str, Dict[str, list]] = {}
    for res in results:
        dst = res["img_metas"]["img_path"].replace(data_root, save_dir)
        seq_dir = os.path.dirname(os.path.dirname(dst))
        img_id = str(int(os.path.splitext(os.path.basename(dst))[0]))
        pred = res["pred"]
        rs = np.asarray(pred["rotations"], dtype=np.float64).reshape(-1, 3, 3)
        ts = np.asarray(pred["translations"], dtype=np.float64).reshape(-1, 3)
        objs = []
        for i, l in enumerate(np.asarray(pred["labels"])):
            d = dict(cam_R_m2c=rs[i].reshape(-1).tolist(), cam_t_m2c=ts[i].tolist(),
                     obj_id=inv.get(int(l) + 1, int(l) + 1))
            if time is not None:
                d["time"] = time
            objs.append(d)
        entries = per_seq.setdefault(seq_dir, {})
        if img_id in entries:
            raise ValueError(f"duplicate image {img_id} in {seq_dir}")
        entries[img_id] = objs
    paths = []
    for seq_dir, content in per_seq.items():
        os.makedirs(seq_dir, exist_ok=True)
        path = os.path.join(seq_dir, "scene_gt.json")
        with open(path, "w") as f:
            f.write(dumps_json(content))
        paths.append(path)
    return paths


# ------------------------------------------------------------------ BOP19 average recall
def load_models_info(path: str) -> Dict[str, dict]:
    """``models_info.json`` of a BOP model folder: {obj_id (str): {diameter, symmetries_discrete,
    symmetries_continuous, …}}."""
    with open(path) as f:
        return {str(k): v for k, v in json.load(f).items()}


def load_depth(path: str, depth_scale: float = 1.0) -> np.ndarray:
    """A BOP depth image (16-bit PNG) as [H, W] float32 in mm: the stored value times the
    camera's ``depth_scale``; 0 stays 0 (no measurement).  PIL is imported here, not at module
    import."""
    try:
        from PIL import Image
    except ImportError as e:  # pragma: no cover
        raise ImportError(f"reading the depth image {path} needs PIL (pillow)") from e
    with Image.open(path) as im:
        d = np.asarray(im)
    if d.ndim != 2:
        raise ValueError(f"{path}: a depth image has one channel, got shape {d.shape}")
    return d.astype(np.float32) * np.float32(depth_scale)


DEPTH_PNG = "{}/depth/{:06d}.png"


GT_INFO_KEYS = ("px_count_all", "px_count_valid", "px_count_visib", "visib_fract", "bbox_obj", "bbox_visib")


def _device_scene_stats(table, labels, frame_index, R, t, K, height, width, depth_test, delta, margin):
    """``scene.scene_visibility``'s stats [n, 12] of one batch of frames as a numpy array."""
    from . import scene
    dev = table.verts.device
    T = lambda a, dt=torch.float32: torch.as_tensor(np.asarray(a)).to(dt).to(dev)  # noqa: E731
    out = scene.scene_visibility(table, T(labels, torch.int32), T(frame_index, torch.int32), T(R), T(t),
                                 T(K), height, width, None if depth_test is None else T(depth_test),
                                 delta, margin, want=("stats",))
    return out["stats"].cpu().numpy()


def compute_gt_info(gt_annots: Dict[str, dict], renderer, depth_root_or_loader=None,
                    delta: float = 15.0, margin: Optional[Tuple[int, int]] = None, *,
                    image_size: Optional[Tuple[int, int]] = None, frames_per_call: int = 32,
                    visibility_fn=None) -> Dict[str, dict]:
    """Fills ``ann['gt_info']`` of every sequence of ``gt_annots`` (``load_bop_annotations``) in the
    shape of ``scene_gt_info.json``: per image a list parallel to ``scene_gt`` of {px_count_all,
    px_count_valid, px_count_visib, visib_fract, bbox_obj, bbox_visib}, computed from the poses and
    the meshes ``renderer`` holds (obj_id = label + 1) by ``scene.scene_visibility`` (DESIGN.md
    §23; the definitions are the project's own, parity with bop_toolkit's calc_gt_info is
    unpinned).  After it ``evaluate_bop`` applies ``min_visib_fract`` as with a shipped file.

    ``depth_root_or_loader``: as for ``evaluate_bop`` (the sensor depth decides visibility), or None:
    mutual occlusion of the annotated instances only, and the frames are ``image_size`` = (H, W)
    (default: the renderer's).  ``margin`` = (x, y): the canvas around the frame on which
    px_count_all and bbox_obj are taken, default (W, H).  ``visibility_fn(table, labels,
    frame_index, R, t, K, H, W, depth_test, delta, margin) → stats [n, 12]`` replaces the device
    call (tests inject a restatement); it gets ``renderer.meshes`` for ``table``."""
    if visibility_fn is None:
        from . import scene
        dev = renderer._device if renderer._device.type == "cuda" else torch.device("cuda")
        table, fn = scene.mesh_table(renderer, dev), _device_scene_stats
    else:
        table, fn = renderer.meshes, visibility_fn
    for seq, ann in gt_annots.items():
        info: Dict[str, list] = {}
        ids = list(ann["pose"])
        for b0 in range(0, len(ids), frames_per_call):
            chunk = ids[b0:b0 + frames_per_call]
            labels, fidx, R, t, K, depth = [], [], [], [], [], []
            for fi, img in enumerate(chunk):
                cam = ann["camera"][img]
                K.append(np.asarray(cam["cam_K"], np.float32).reshape(3, 3))
                if callable(depth_root_or_loader):
                    depth.append(np.asarray(depth_root_or_loader(seq, int(img)), np.float32))
                elif depth_root_or_loader is not None:
                    depth.append(load_depth(osp.join(depth_root_or_loader, DEPTH_PNG.format(seq, int(img))),
                                            float(cam.get("depth_scale", 1.0))))
                for obj in ann["pose"][img]:
                    labels.append(int(obj["obj_id"]) - 1)
                    fidx.append(fi)
                    R.append(np.asarray(obj["cam_R_m2c"], np.float32).reshape(3, 3))
                    t.append(np.asarray(obj["cam_t_m2c"], np.float32).reshape(3))
            if depth:
                if any(d.shape != depth[0].shape for d in depth):
                    raise ValueError(f"sequence {seq}: the frames differ in size")
                h, w = depth[0].shape
            else:
                h, w = image_size if image_size is not None else renderer.image_size
            n = len(labels)
            stats = np.zeros((0, 12), np.int64)
            if n:
                stats = np.asarray(fn(table, np.asarray(labels, np.int32), np.asarray(fidx, np.int32),
                                      np.stack(R), np.stack(t), np.stack(K), int(h), int(w),
                                      np.stack(depth) if depth else None, float(delta),
                                      (int(w), int(h)) if margin is None else tuple(margin)))
            k = 0
            for img in chunk:
                rows = []
                for _ in ann["pose"][img]:
                    s = [int(v) for v in stats[k]]
                    rows.append(dict(px_count_all=s[0], px_count_valid=s[1], px_count_visib=s[2],
                                     visib_fract=s[2] / s[0] if s[0] > 0 else 0.0,
                                     bbox_obj=s[3:7], bbox_visib=s[7:11]))
                    k += 1
                info[img] = rows
        ann["gt_info"] = info
    return gt_annots


def write_gt_info(root: str, gt_annots: Dict[str, dict]) -> List[str]:
    """``ann['gt_info']`` of every sequence as '{root}/{sequence:06d}/scene_gt_info.json' (where
    ``load_bop_annotations`` reads it); returns the written paths."""
    paths = []
    for seq, ann in gt_annots.items():
        path = osp.join(root, INFO_JSON.format(int(seq)))
        os.makedirs(osp.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(dumps_json(ann["gt_info"]))
        paths.append(path)
    return paths


def _device_bop_errors(batch: dict, renderer):
    """The three error functions of the matched pairs on the device (``bop_metrics``)."""
    from . import bop_metrics as bm
    from .patches import point_table
    dev = renderer._device if renderer._device.type == "cuda" else torch.device("cuda")
    T = lambda a, dt=torch.float32: torch.as_tensor(np.asarray(a)).to(dt).to(dev)  # noqa: E731
    points, counts = point_table(renderer)
    num_classes = points.shape[0]
    table, offset = bm.symmetry_table(batch["models_info"], num_classes, dev)
    lab = T(batch["labels"], torch.int64)
    args = [T(batch[k]) for k in ("R_est", "t_est", "R_gt", "t_gt")]
    K = T(batch["K"])
    mssd, mspd = bm.mssd_mspd(points.to(dev), counts.to(dev), table, offset, lab, *args, K)
    e = bm.vsd(renderer, lab, *args, K, T(batch["depth_test"]), T(batch["frame_index"], torch.int32),
               T(batch["diameters"]), batch["taus"], batch["delta"])
    return e.cpu().numpy(), mssd.double().cpu().numpy(), mspd.double().cpu().numpy()


def evaluate_bop(results: Sequence[dict], gt_annots: Dict[str, dict], models_info: Dict[str, dict],
                 renderer, depth_root_or_loader, class_names: Optional[Sequence[str]] = None,
                 inverse_label_mapping: Optional[Dict[int, int]] = None,
                 match_points: Optional[Sequence[np.ndarray]] = None,
                 taus: Optional[Sequence[float]] = None, delta: Optional[float] = None,
                 min_visib_fract: float = 0.1, error_fn=None) -> Dict[str, float]:
    """BOP19 average recall of ``results`` → the flat '{name}/{metric}' dictionary: 'all/AR',
    'all/AR_VSD', 'all/AR_MSSD', 'all/AR_MSPD' over every target, the per-threshold recalls
    'all/mssd_05' … 'all/mssd_50' and 'all/mspd_05' … 'all/mspd_50', and with ``class_names``
    '{class}/AR…' over that class's targets (−1 for a class without a target).

    ``match_results`` pairs one estimate with every GT instance; its errors are VSD, MSSD and MSPD
    (``bop_metrics``), a GT without an estimate has +inf errors, and ``average_recall`` thresholds
    them.  Targets: the GT instances with ``visib_fract`` ≥ ``min_visib_fract`` where the
    annotations hold ``scene_gt_info``, otherwise every GT instance.  bop_toolkit matches estimates
    to GTs greedily by score; this keeps ``match_results``' one estimate per GT — the refiner emits
    one estimate per detection with score 1, where the two coincide; with several estimates per
    instance they do not (unpinned, as is every parity with the toolkit itself: it is absent).

    ``models_info``: ``load_models_info`` (diameters and symmetries; obj_id = label + 1).
    ``renderer``: a ``Renderer`` holding the classes' meshes, at least as large as the frames; its
    vertices are the error functions' model points (and ``match_points``' default).
    ``depth_root_or_loader``: a callable ``(sequence, image id) → [H, W]`` depth in mm, or the
    dataset root, read as '{root}/{sequence}/depth/{image:06d}.png' times the camera's
    ``depth_scale``.  All frames have one size.  ``error_fn(batch, renderer) → (vsd [M, n_taus],
    mssd [M], mspd [M])`` replaces the device computation (tests inject a restatement)."""
    from . import bop_metrics as bm
    taus = bm.BOP19_TAUS if taus is None else tuple(taus)
    delta = bm.BOP19_DELTA if delta is None else float(delta)
    num_classes = max(renderer.meshes) + 1
    diam_of = [float((models_info.get(str(l + 1)) or {}).get("diameter", 1.0)) for l in range(num_classes)]
    symmetric = [l for l in range(num_classes)
                 if (models_info.get(str(l + 1)) or {}).get("symmetries_discrete")
                 or (models_info.get(str(l + 1)) or {}).get("symmetries_continuous")]
    if match_points is None:
        match_points = [renderer.meshes[l][0].cpu().numpy() if l in renderer.meshes
                        else np.zeros((1, 3), np.float32) for l in range(num_classes)]
    gR, gT, pR, pT, labels, valid, K = match_results(results, gt_annots, match_points, symmetric, diam_of,
                                                     inverse_label_mapping)
    # the walk of match_results once more: the frame and the visibility of every GT instance
    frames, frame_index, targets = [], [], []
    for fi, res in enumerate(results):
        seq, img_id = _seq_and_image(res["img_metas"]["img_path"])
        ann = gt_annots[seq]
        if callable(depth_root_or_loader):
            d = np.asarray(depth_root_or_loader(seq, img_id), np.float32)
        else:
            scale = float(ann["camera"][str(img_id)].get("depth_scale", 1.0))
            d = load_depth(osp.join(depth_root_or_loader, DEPTH_PNG.format(seq, img_id)), scale)
        if frames and d.shape != frames[0].shape:
            raise ValueError(f"frame {seq}/{img_id} is {d.shape}, the first one {frames[0].shape}")
        frames.append(d)
        info = ann.get("gt_info", {}).get(str(img_id))
        for k in range(len(ann["pose"][str(img_id)])):
            frame_index.append(fi)
            targets.append(True if info is None else float(info[k]["visib_fract"]) >= min_visib_fract)
    frame_index, targets = np.asarray(frame_index, np.int32), np.asarray(targets, bool)
    m = labels.shape[0]
    diam = np.asarray([diam_of[l] for l in labels], np.float64)
    vsd_e = np.full((m, len(taus)), np.inf)
    mssd_e, mspd_e = np.full(m, np.inf), np.full(m, np.inf)
    if valid.any():
        batch = dict(labels=labels[valid], R_est=pR[valid], t_est=pT[valid], R_gt=gR[valid], t_gt=gT[valid],
                     K=K[valid], depth_test=np.stack(frames), frame_index=frame_index[valid],
                     diameters=diam[valid].astype(np.float32), models_info=models_info, taus=taus,
                     delta=delta)
        v, s, p = (error_fn or _device_bop_errors)(batch, renderer)
        vsd_e[valid], mssd_e[valid], mspd_e[valid] = v, s, p
    width = frames[0].shape[1]
    out: Dict[str, float] = {}

    def put(name, sel):
        if not (targets & sel).any():
            out.update({f"{name}/{k}": -1.0 for k in ("AR", "AR_VSD", "AR_MSSD", "AR_MSPD")})
            return None
        ar = bm.average_recall(vsd_e, mssd_e, mspd_e, diam, width, targets & sel)
        out.update({f"{name}/{k}": ar[k] for k in ("AR", "AR_VSD", "AR_MSSD", "AR_MSPD")})
        return ar
    ar = put("all", np.ones(m, bool))
    if ar is not None:
        for i, th in enumerate(bm.BOP19_THETAS):
            out["all/mssd_{:0>2d}".format(int(round(th * 100)))] = float(ar["recall_mssd"][i])
        for i, th in enumerate(bm.BOP19_MSPD_THETAS):
            out["all/mspd_{:0>2d}".format(int(th))] = float(ar["recall_mspd"][i])
    for l, name in enumerate(class_names or ()):
        put(name, labels == l)
    return out
