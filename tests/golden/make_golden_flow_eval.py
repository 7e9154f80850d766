"""Fixture of the flow-validation functions from the REFERENCE's own code (``models/utils/pose.py``
get_flow_from_delta_pose_and_depth, ``models/utils/flow.py`` filter_flow_by_mask /
filter_flow_by_depth / filter_flow_by_face_index / cal_epe, ``models/utils/warp.py`` coords_grid),
loaded with ``make_golden``'s shims, run in float64 on the CPU.

    python tests/golden/make_golden_flow_eval.py

writes ``golden_flow_eval.npz``.  The inputs are regenerated from seeds by the tests
(``tests/flow_eval_restatement.py`` ``scene_case`` / ``epe_case`` / ``mark_invalid``); the fixture
stores, for the batch ``scene_case('fixture')`` = ``synthetic.make_train_batch(4, 64, 3)`` with the
GT pose's ``ellipsoid_depth`` and a synthetic face-index map with its shifted copy:

* the invalid pixels (both channels equal to ``invalid_num``) of the GT flow and of every filter's
  output, packed to bits: the mask filter, the depth filter as the reference writes it (on
  ``mark_invalid(flow)``, whose already-invalid pixels above ``invalid_num`` make the ``&``
  observable), the face-index filter, and the three one after another;
* the depth filter's ``consistent`` map, evaluated with the reference's ``coords_grid`` and the
  statements of flow.py:33-40 (the reference has no function that returns it): what the
  ``combine='or'`` mode is checked against;
* sums and absolute sums of the flows, ``cal_epe``'s 'total_mean', 'none' and 'mean'['mean'] with
  and without a mask;
* per ``epe_case`` (the three shapes of the GPU tests) the deviation of the reference's own float32
  CPU run of ``cal_epe`` from its float64 run on the same float32 inputs — 'total_mean' mean, the
  largest 'mean'['mean'] deviation, the largest 'none' deviation: a quarter of the GPU tests' gates.

The generator refuses to write unless the mask filter removes between 2 % and 50 % of the valid
pixels and at most 1 % of the pixels are near a decision (``flow_eval_restatement``'s margins).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import flow_eval_restatement as fr  # noqa: E402

NAME = "golden_flow_eval"
INVALID, THR = 400.0, 0.2
MASK_REMOVES, NEAR_MAX = (0.02, 0.50), 0.01


def load():
    ref = mg.load_reference()
    mg._load("models.utils.warp", "models/utils/warp.py")
    ref.flow = mg._load("models.utils.flow", "models/utils/flow.py")
    ref.warp = sys.modules["models.utils.warp"]
    return ref


def invalid_bits(flow):
    return np.packbits(((flow[:, 0] == INVALID) & (flow[:, 1] == INVALID)).numpy())


def consistent_map(ref, flow, depth1, depth0):
    """flow.py:33-40 with the reference's coords_grid."""
    d1 = torch.where(depth1 > 0, depth1, torch.zeros_like(depth1))
    d0 = torch.where(depth0 > 0, depth0, torch.zeros_like(depth0))
    warped = torch.nn.functional.grid_sample(d1[:, None], ref.warp.coords_grid(flow).double(),
                                             padding_mode="zeros", mode="bilinear", align_corners=True)
    return (((d0[:, None] - warped).abs() / (d0[:, None] + 0.1)) < THR)[:, 0]


def epe_deviation(ref, name):
    """|float32 run − float64 run| of the reference's cal_epe on one epe_case's float32 inputs."""
    tgt, pred, mask, _ = fr.epe_case(name)
    dev = np.zeros(3)
    for m in (None, mask):
        r32 = [ref.flow.cal_epe(tgt.clone(), pred.clone(), m, INVALID, red) for red in ("total_mean", "mean", "none")]
        r64 = [ref.flow.cal_epe(tgt.double(), pred.double(), None if m is None else m.double(), INVALID, red)
               for red in ("total_mean", "mean", "none")]
        dev[0] = max(dev[0], abs(float(r32[0]["mean"].double() - r64[0]["mean"])))
        dev[1] = max(dev[1], float((r32[1]["mean"].double() - r64[1]["mean"]).abs().max()))
        dev[2] = max(dev[2], float((r32[2].double() - r64[2]).abs().max()))
    return dev


def main():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    ref = load()
    b = fr.scene_case("fixture")
    dd = {k: v.double() for k, v in b.items() if v.is_floating_point()}
    flow = ref.pose.get_flow_from_delta_pose_and_depth(
        dd["ref_rotation"], dd["ref_translation"], dd["gt_rotation"], dd["gt_translation"],
        dd["depth"], dd["internel_k"], invalid_num=INVALID)
    assert flow.dtype == torch.float64
    f_mask = ref.flow.filter_flow_by_mask(flow.clone(), b["gt_masks"], INVALID)
    marked = fr.mark_invalid(flow)
    f_depth = ref.flow.filter_flow_by_depth(marked.clone(), dd["gt_depth"], dd["depth"], INVALID, THR)
    # the face-index filter samples a float32 map, so its grid — the flow — must be float32 too
    f_face = ref.flow.filter_flow_by_face_index(flow.float(), b["face_index"], b["gt_face_index"], INVALID)
    f_all = ref.flow.filter_flow_by_face_index(
        ref.flow.filter_flow_by_depth(
            ref.flow.filter_flow_by_mask(flow.clone(), b["gt_masks"], INVALID),
            dd["gt_depth"], dd["depth"], INVALID, THR).float(),
        b["face_index"], b["gt_face_index"], INVALID)
    cons = consistent_map(ref, flow, dd["gt_depth"], dd["depth"])

    # refusals
    valid0 = ~((flow[:, 0] == INVALID) & (flow[:, 1] == INVALID))
    valid1 = ~((f_mask[:, 0] == INVALID) & (f_mask[:, 1] == INVALID))
    removed = 1.0 - float(valid1.sum()) / float(valid0.sum())
    pred = fr.pred_flow(f_mask.float(), 0)
    st = fr.epe_stats(f_mask.float(), pred, None, INVALID)
    near = (fr.mask_filter(flow, b["gt_masks"], INVALID)[1] |
            fr.depth_filter(flow, b["gt_depth"], b["depth"], INVALID, THR)[1] |
            fr.face_filter(flow, b["face_index"], b["gt_face_index"], INVALID)[1] | st["near"])
    near_share = float(near.double().mean())
    print(f"valid {float(valid0.double().mean()):.3f} of the pixels, {float(valid1.double().mean()):.3f} "
          f"after the mask filter (removes {removed:.3f}); near a decision: {int(near.sum())} pixels "
          f"({near_share:.4f})")
    assert MASK_REMOVES[0] <= removed <= MASK_REMOVES[1], f"mask filter removes {removed}"
    assert near_share <= NEAR_MAX, f"{near_share} of the pixels are near a decision"
    assert int((f_depth != marked).any(1).sum()) > 0, "the reference's & is not observable"

    out = dict(meta=np.array([fr.FIXTURE["batch"], fr.FIXTURE["size"], fr.FIXTURE["seed"]]),
               invalid_num=np.array(INVALID), depth_thr=np.array(THR),
               removed=np.array(removed), near_share=np.array(near_share),
               bits_flow=invalid_bits(flow), bits_mask=invalid_bits(f_mask),
               bits_depth_reference=invalid_bits(f_depth), bits_face=invalid_bits(f_face),
               bits_all_reference=invalid_bits(f_all), bits_consistent=np.packbits(cons.numpy()),
               depth_rewritten=np.array(int((f_depth != marked).any(1).sum())))
    for tag, f in (("flow", flow), ("mask", f_mask), ("depth_reference", f_depth), ("face", f_face),
                   ("all_reference", f_all)):
        out[f"sum_{tag}"] = np.array([float(f.sum()), float(f.abs().sum())])
    tgt, pred, mask, _ = fr.epe_case("fixture")
    for tag, m in (("nomask", None), ("mask", mask.double())):
        tm = ref.flow.cal_epe(tgt.double(), pred.double(), m, INVALID, "total_mean")
        out[f"epe_total_mean_{tag}"] = np.array([float(tm[k]) for k in ("mean", "1px", "3px", "5px")])
        out[f"epe_mean_{tag}"] = ref.flow.cal_epe(tgt.double(), pred.double(), m, INVALID, "mean")["mean"].numpy()
        out[f"epe_none_{tag}"] = ref.flow.cal_epe(tgt.double(), pred.double(), m, INVALID, "none").numpy()
    for name in fr.CASES:
        out[f"dev_{name}"] = epe_deviation(ref, name)
        print(f"float32 vs float64 cal_epe, case {name}: total mean {out[f'dev_{name}'][0]:.3e} px, "
              f"per-sample mean {out[f'dev_{name}'][1]:.3e} px, map {out[f'dev_{name}'][2]:.3e} px")
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{NAME}.npz: {size} bytes")
    assert size <= 1 << 20


if __name__ == "__main__":
    main()
