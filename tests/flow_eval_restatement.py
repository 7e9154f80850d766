"""fp64 restatement of the flow-validation semantics (scflow_amd/flow_eval.py) on the
CPU, and the inputs the flow-validation tests and ``golden/make_golden_flow_eval.py`` share.

Every function takes torch tensors of any float dtype and computes in float64.  A filter returns
``(bad, near)``: the pixels it rewrites with ``invalid_num``, and the pixels whose decision is
within the near-decision margin of the issue (mask sample within 1e-4 of 0.9, depth ratio within
1e-4 of the threshold, a nearest-sample coordinate within 1e-3 of a half) — where an fp32
implementation may legitimately decide the other way.  ``epe_stats`` likewise flags ``|flow|``
within 1e-3 of ``max_flow`` and an error within 1e-3 px of a threshold.
"""
import numpy as np
import torch
import torch.nn.functional as F

from scflow_amd import synthetic

NEAR_MASK, NEAR_RATIO, NEAR_HALF, NEAR_PX = 1e-4, 1e-4, 1e-3, 1e-3
FIXTURE = dict(batch=4, size=64, seed=3)  # the batch of golden_flow_eval.npz
ABOVE = 450.0  # what mark_invalid writes: above the default invalid_num


def d64(x):
    return torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).double()


# ------------------------------------------------------------------------------------ inputs
def _scene(batch, size, seed, rows=None, zero=None):
    """``synthetic.make_train_batch`` plus the GT pose's depth (``synthetic.ellipsoid_depth``) and
    the two face-index maps (a 4×4-block index map of the rendered object, 0 on the background,
    and a copy shifted by (+1 row, −2 columns)), as torch tensors.  ``rows`` = (r0, r1) keeps
    those image rows (a non-square image; the principal point moves with it); ``zero``: a sample
    whose rendered depth is zero everywhere."""
    b = synthetic.make_train_batch(batch, size, seed=seed)
    gt_depth = []
    for i in range(batch):
        d_obj = synthetic.YCBV_DIAMETERS[int(b["label"][i]) % len(synthetic.YCBV_DIAMETERS)]
        gt_depth.append(synthetic.ellipsoid_depth(
            b["gt_rotation"][i].astype(np.float64), b["gt_translation"][i].astype(np.float64),
            b["internel_k"][i].astype(np.float64), size, np.array(synthetic.ELLIPSOID_AXES) * d_obj))
    b["gt_depth"] = np.stack(gt_depth).astype(np.float32)
    if zero is not None:
        b["depth"][zero] = 0.0
    if rows is not None:
        for k in ("depth", "gt_depth", "gt_masks"):
            b[k] = b[k][:, rows[0]:rows[1]]
        b["internel_k"] = b["internel_k"].copy()
        b["internel_k"][:, 1, 2] -= rows[0]
    h, w = b["depth"].shape[1:]
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    blocks = ((yy // 4) * ((w + 3) // 4) + xx // 4 + 1).astype(np.int64)
    face1 = np.where(b["depth"] > 0, blocks[None], 0)
    b["face_index"] = face1
    b["gt_face_index"] = np.roll(face1, shift=(1, -2), axis=(1, 2))
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in b.items()}


CASES = ("fixture", "rect", "tiny")


def scene_case(name):
    """The three shapes of the GPU tests: 'fixture' (N = 4, 64², the golden batch), 'rect' (N = 3,
    H = 20, W = 36: non-square, H·W no multiple of 256, sample 1 without any depth) and 'tiny'
    (N = 1, 8²)."""
    if name == "fixture":
        return _scene(**FIXTURE)
    if name == "rect":
        return _scene(3, 36, seed=5, rows=(8, 28), zero=1)
    assert name == "tiny"
    return _scene(1, 8, seed=7)


def scene_gt_flow(b, invalid_num=400.0):
    return gt_flow(b["depth"], b["internel_k"], b["ref_rotation"], b["ref_translation"],
                   b["gt_rotation"], b["gt_translation"], invalid_num)


def epe_case(name, seed=0):
    """(flow_tgt, flow_pred, mask, occ_pred), float32, of a scene case: the restated GT flow
    filtered by the GT mask, ``pred_flow`` of it, the rendered mask and ``occ_pred``."""
    b = scene_case(name)
    flow = scene_gt_flow(b)
    tgt = apply_filter(flow, mask_filter(flow, b["gt_masks"])[0]).float()
    return tgt, pred_flow(tgt, seed), (b["depth"] > 0).float(), occ_pred(tuple(b["depth"].shape), seed)


def pred_flow(flow, seed, sigma=2.5):
    """A prediction for ``flow`` [N, 2, H, W]: the flow plus N(0, sigma) noise (errors on both sides
    of 1, 3 and 5 px) where it is below 100 px, plain noise elsewhere; float32."""
    rng = np.random.default_rng(seed + 611953)
    f = flow.detach().cpu().double().numpy()
    noise = rng.normal(0.0, sigma, f.shape)
    return torch.from_numpy(np.where(np.abs(f) < 100.0, f + noise, noise).astype(np.float32))


def occ_pred(shape, seed):
    rng = np.random.default_rng(seed + 32452843)
    return torch.from_numpy(rng.uniform(0.0, 1.0, shape).astype(np.float32))


def mark_invalid(flow, value=ABOVE):
    """A copy of ``flow`` with the pixels (7x + 3y) % 11 == 0 set to ``value`` in both channels:
    already-invalid pixels ABOVE invalid_num, on the object too — what makes the reference's
    ``not_valid & ~consistent`` observable."""
    n, _, h, w = flow.shape
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    sel = ((7 * xx + 3 * yy) % 11 == 0).to(flow.device)
    out = flow.clone()
    out[:, :, sel] = value
    return out


# ------------------------------------------------------------------------------------ GT flow
def gt_flow(depth, K, R_ref, t_ref, R_gt, t_gt, invalid_num=400.0):
    """get_flow_from_delta_pose_and_depth, dense: lift the pixels with depth > 0 by (K, R_ref,
    t_ref), project by (K, R_gt, t_gt); ``invalid_num`` elsewhere."""
    depth, K, R_ref, t_ref, R_gt, t_gt = map(d64, (depth, K, R_ref, t_ref, R_gt, t_gt))
    n, h, w = depth.shape
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64),
                            torch.arange(w, dtype=torch.float64), indexing="ij")
    homo = torch.stack([xx, yy, torch.ones_like(xx)], -1).view(1, h * w, 3) * depth.view(n, h * w, 1)
    cam = homo @ torch.linalg.inv(K).transpose(1, 2)
    obj = (cam - t_ref[:, None]) @ torch.linalg.inv(R_ref).transpose(1, 2)
    dst = (obj @ R_gt.transpose(1, 2) + t_gt[:, None]) @ K.transpose(1, 2)
    z = torch.where(dst[..., 2] == 0, torch.ones_like(dst[..., 2]), dst[..., 2])
    fx = (dst[..., 0] / z).view(n, h, w) - xx
    fy = (dst[..., 1] / z).view(n, h, w) - yy
    flow = torch.stack([fx, fy], 1)
    return torch.where((depth > 0)[:, None], flow, torch.full_like(flow, float(invalid_num)))


def _grid(flow):
    """coords_grid (models/utils/warp.py): normalised with max(size − 1, 1) for every sampler."""
    n, _, h, w = flow.shape
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64),
                            torch.arange(w, dtype=torch.float64), indexing="ij")
    gx = (xx + flow[:, 0]) * 2.0 / max(w - 1, 1) - 1.0
    gy = (yy + flow[:, 1]) * 2.0 / max(h - 1, 1) - 1.0
    return torch.stack([gx, gy], -1)


def _bad0(flow, invalid_num):
    return (flow[:, 0] >= invalid_num) & (flow[:, 1] >= invalid_num)


def mask_filter(flow, gt_mask, invalid_num=400.0):
    flow = d64(flow)
    m = F.grid_sample(d64(gt_mask)[:, None], _grid(flow), mode="bilinear", padding_mode="zeros",
                      align_corners=False)[:, 0]
    return (m < 0.9) | _bad0(flow, invalid_num), (m - 0.9).abs() < NEAR_MASK


def depth_filter(flow, depth1, depth0, invalid_num=400.0, thr=0.2, combine="or"):
    assert combine in ("or", "reference")
    flow, depth1, depth0 = d64(flow), d64(depth1), d64(depth0)
    d1 = torch.where(depth1 > 0, depth1, torch.zeros_like(depth1))
    d0 = torch.where(depth0 > 0, depth0, torch.zeros_like(depth0))
    warped = F.grid_sample(d1[:, None], _grid(flow), mode="bilinear", padding_mode="zeros",
                           align_corners=True)[:, 0]
    ratio = (d0 - warped).abs() / (d0 + 0.1)
    consistent = ratio < thr
    bad0 = _bad0(flow, invalid_num)
    bad = (bad0 | ~consistent) if combine == "or" else (bad0 & ~consistent)
    return bad, (ratio - thr).abs() < NEAR_RATIO


def face_filter(flow, face_index1, face_index2, invalid_num=400.0):
    flow = d64(flow)
    f1, f2 = face_index1.float().double(), face_index2.float().double()  # compared as float32
    g = _grid(flow)
    s = F.grid_sample(f2[:, None], g, mode="nearest", padding_mode="zeros", align_corners=True)[:, 0]
    n, _, h, w = flow.shape
    near = torch.zeros(n, h, w, dtype=torch.bool)
    for c, size in ((0, w), (1, h)):
        pix = (g[..., c] + 1.0) / 2.0 * (size - 1)
        near |= ((pix - torch.floor(pix)) - 0.5).abs() < NEAR_HALF
    return (s != f1) | _bad0(flow, invalid_num), near


def apply_filter(flow, bad, invalid_num=400.0):
    """Out of place: ``invalid_num`` in both channels where ``bad``."""
    return torch.where(bad[:, None], torch.full_like(flow, float(invalid_num)), flow)


# ------------------------------------------------------------------------------------ EPE
def epe_stats(flow_tgt, flow_pred, mask=None, max_flow=400.0, threshs=(1, 3, 5), occ_pred=None):
    """The per-sample statistics of scflow_flow_epe: count, below [N, 3], err_sum, occ_sum, the
    masked error map, the validity map and the near-decision map."""
    tgt, pred = d64(flow_tgt), d64(flow_pred)
    mag = (tgt ** 2).sum(1).sqrt()
    inside = mag < max_flow
    valid = inside if mask is None else inside & (d64(mask).reshape(inside.shape) >= 0.5)
    err = ((tgt - pred) ** 2).sum(1).sqrt()
    near = (mag - max_flow).abs() < NEAR_PX
    for t in threshs:
        near |= valid & ((err - t).abs() < NEAR_PX)
    out = dict(count=valid.sum((1, 2)), err_sum=(err * valid).sum((1, 2)),
               below=torch.stack([(valid & (err < t)).sum((1, 2)) for t in threshs], 1),
               error_map=err * valid, valid=valid, inside=inside, near=near)
    if occ_pred is not None:
        out["occ_sum"] = (inside.double() - d64(occ_pred).reshape(inside.shape)).abs().sum((1, 2))
    return out


def cal_epe(flow_tgt, flow_pred, mask, max_flow=400.0, reduction="mean", threshs=(1, 3, 5)):
    """cal_epe (models/utils/flow.py:64-88) with the 'mean' branch's ``…px`` entries over the valid
    pixels (the deviation flow_eval.py documents)."""
    st = epe_stats(flow_tgt, flow_pred, mask, max_flow, threshs)
    if reduction == "none":
        return st["error_map"]
    if reduction == "total_mean":
        total = st["count"].sum().double() + 1e-10
        out = dict(mean=st["err_sum"].sum() / total)
        out.update({f"{t}px": st["below"][:, k].sum().double() / total for k, t in enumerate(threshs)})
        return out
    assert reduction == "mean"
    total = st["count"].double() + 1e-10
    out = dict(mean=st["err_sum"] / total)
    out.update({f"{t}px": st["below"][:, k].double() / total for k, t in enumerate(threshs)})
    return out


def eval_epe_and_occ(batch_flow, batch_occlusion, flow, noc_flow, max_flow=400.0,
                     reduction="total_mean", noc_without_mask=False, prefix="epe"):
    """eval_epe_and_occ (raft_refiner_flow_mask.py:239-259) against a GT flow and its mask-filtered
    form (None without a GT mask)."""
    out = {f"{prefix}_{k}": v for k, v in cal_epe(flow, batch_flow, None, max_flow, reduction).items()}
    if noc_flow is not None:
        out.update({f"{prefix}_noc_{k}": v
                    for k, v in cal_epe(noc_flow, batch_flow, None, max_flow, reduction).items()})
    elif noc_without_mask:
        out.update({f"{prefix}_noc_{k[len(prefix) + 1:]}": v for k, v in list(out.items())})
    if batch_occlusion is not None:
        tgt = d64(noc_flow if noc_flow is not None else flow)
        occ_gt = ((tgt ** 2).sum(1).sqrt() < max_flow).double()
        out["occ"] = (occ_gt - d64(batch_occlusion).reshape(occ_gt.shape)).abs().mean()
    return out
