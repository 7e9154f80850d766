"""Shared inputs of the RANSAC-PnP tests: synthetic scenes with a known ground-truth pose, the
oracle's lift and ground-truth flow, and the contaminated flow.  Built once per shape and shared
(the returned arrays are read-only)."""
from functools import lru_cache

import numpy as np
import torch

from scflow_amd import synthetic
from tests import pnp_restatement as pr

# (B, H, W, seed, index of a sample whose depth is all zero or None)
CASE_SQUARE = (3, 64, 64, 3, 2)
CASE_WIDE = (2, 48, 80, 5, None)   # non-square: strides and tails
CASE_LARGE = (2, 256, 256, 7, None)  # several point chunks per sample


@lru_cache(maxsize=None)
def case(B, H, W, seed, empty):
    """dict of float32 numpy arrays: depth [B, H, W], K, R_ref, t_ref, R_gt, t_gt, points
    [B, H, W, 4] (the oracle's lift + validity), flow (the oracle's ground-truth flow, computed in
    fp64 and rounded once), flow_c / moved (30 % of the valid pixels moved by 10-40 px)."""
    import oracle.scflow_oracle as orc
    S = max(H, W)
    sc = synthetic.make_scene(B, S, seed=seed)
    tg = synthetic.make_train_targets(sc, S, seed=seed)
    depth = sc["depth"][:, :H, :W].copy()
    if empty is not None:
        depth[empty] = 0.0
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    K, R0, t0 = sc["internel_k"], sc["ref_rotation"], sc["ref_translation"]
    R1, t1 = tg["gt_rotation"], tg["gt_translation"]
    pts, valid = orc.lift_points(T(depth), T(K), T(R0), T(t0))
    points = torch.cat([pts, valid[..., None].float()], -1).numpy()
    flow = orc.flow_from_delta_pose_and_depth(T(R0).double(), T(t0).double(), T(R1).double(),
                                              T(t1).double(), T(depth).double(), T(K).double(),
                                              invalid_num=0.0).float().numpy()
    flow_c, moved = pr.contaminate(flow, depth > 0, frac=0.3, seed=seed)
    out = dict(depth=depth, K=K, R_ref=R0, t_ref=t0, R_gt=R1, t_gt=t1, points=points, flow=flow,
               flow_c=flow_c, moved=moved)
    for v in out.values():
        v.setflags(write=False)
    return out
