"""CPU: the BOP19 pose errors' host side (``scflow_amd.bop_metrics``, the additions to
``scflow_amd.bop_eval``) and the float64 restatement the GPU tests compare the kernels with
(``tests/bop_restatement.py``): symmetry sets, closed forms of MSSD / MSPD / VSD, recall on a
hand-worked table, the file readers, ``evaluate_bop``'s keys, and the two conditions the GPU tests
lean on — ambiguous pixels ≤ 1 % of the union in every committed VSD case, and the end-to-end
perturbations away from every threshold by more than the fp32 tolerances."""
import json
import math

import numpy as np
import pytest

from scflow_amd import bop_eval, bop_metrics as bm
from tests import bop_cases as bc
from tests import bop_restatement as br

AXIS, OFFSET = [0.3, -0.5, 0.8], [4.0, -7.0, 2.5]
DISC_X = [1.0, 0, 0, 0, 0, -1.0, 0, 0, 0, 0, -1.0, 0, 0, 0, 0, 1.0]      # 180° about x
DISC_Y = [-1.0, 0, 0, 2.0, 0, 1.0, 0, 0, 0, 0, -1.0, 6.0, 0, 0, 0, 1.0]  # 180° about y through (1, ·, 3)


# ------------------------------------------------------------------------------ symmetry sets
def test_continuous_axis_gives_315_rigid_transforms_about_the_offset():
    t = bm.symmetry_transforms({"symmetries_continuous": [{"axis": AXIS, "offset": OFFSET}]})
    assert t.shape == (315, 3, 4) and t.dtype == np.float64
    R, tr = t[:, :, :3], t[:, :, 3]
    assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() <= 1e-12
    assert np.abs(np.linalg.det(R) - 1.0).max() <= 1e-12
    off = np.array(OFFSET)
    assert np.abs(R @ off + tr - off).max() <= 1e-12   # the offset is a fixed point
    assert np.array_equal(t[0], np.eye(3, 4))
    a = np.array(AXIS) / np.linalg.norm(AXIS)
    assert np.abs(R @ a - a).max() <= 1e-12            # rotations about the axis
    ang = np.arccos(np.clip((np.trace(R[1]) - 1) / 2, -1, 1))
    assert abs(ang - 2 * math.pi / 315) <= 1e-9


def test_symmetry_set_sizes():
    cont = [{"axis": AXIS, "offset": OFFSET}]
    assert bm.symmetry_transforms({"symmetries_discrete": [DISC_X, DISC_Y],
                                   "symmetries_continuous": cont}).shape[0] == 3 * 315
    d = bm.symmetry_transforms({"symmetries_discrete": [DISC_X, DISC_Y]})
    assert d.shape == (3, 3, 4) and np.array_equal(d[0], np.eye(3, 4))
    assert np.array_equal(d[2], np.array(DISC_Y).reshape(4, 4)[:3])
    for none in (None, {}, {"diameter": 3.0}):
        assert np.array_equal(bm.symmetry_transforms(none), np.eye(3, 4)[None])
    assert bm.symmetry_transforms({"symmetries_continuous": cont}, max_sym_disc_step=0.1).shape[0] == 32


@pytest.mark.parametrize("s", sorted(bc.SYM_KINDS))
def test_symmetry_transforms_match_the_restatement(s):
    t = bm.symmetry_transforms(bc.SYM_KINDS[s])
    ref = br.symmetry_set(bc.SYM_KINDS[s])
    assert t.shape[0] == len(ref) == s
    for a, (R, tr) in zip(t, ref):
        assert np.abs(a[:, :3] - R).max() <= 1e-12 and np.abs(a[:, 3] - tr).max() <= 1e-12


# ------------------------------------------------------------------------------ MSSD / MSPD
def test_mssd_of_a_symmetric_copy_is_zero():
    rng = np.random.default_rng(0)
    verts = rng.uniform(-80, 80, (50, 3))
    syms = br.symmetry_set({"symmetries_discrete": [DISC_Y],
                            "symmetries_continuous": [{"axis": AXIS, "offset": OFFSET}]}, step=0.2)
    Rg, tg = bc._random_rotation(rng), np.array([30.0, -20.0, 900.0])
    for Rs, ts in syms:  # est = GT∘S
        assert br.mssd(Rg @ Rs, Rg @ ts + tg, Rg, tg, verts, syms) <= 1e-9
    assert br.mssd(Rg @ syms[3][0], Rg @ syms[3][1] + tg, Rg, tg, verts, syms[:1]) > 1.0


def test_mssd_of_a_rotation_about_an_axis_through_the_origin():
    rng = np.random.default_rng(1)
    verts = rng.uniform(-80, 80, (40, 3))
    a = np.array(AXIS) / np.linalg.norm(AXIS)
    theta = 0.37
    t = np.array([5.0, 6.0, 700.0])
    far = np.linalg.norm(verts - np.outer(verts @ a, a), axis=1).max()
    got = br.mssd(br.rot_axis_angle(a, theta), t, np.eye(3), t, verts, [(np.eye(3), np.zeros(3))])
    assert abs(got - 2 * math.sin(theta / 2) * far) <= 1e-9


def test_mspd_of_a_planar_shift():
    rng = np.random.default_rng(2)
    verts = np.concatenate([rng.uniform(-80, 80, (30, 2)), np.zeros((30, 1))], 1)  # object z = 0
    Z, d, fx = 850.0, 12.0, 1066.778
    got = br.mspd(np.eye(3), [d, 0, Z], np.eye(3), [0, 0, Z], bc.CAM_K, verts, [(np.eye(3), np.zeros(3))])
    assert abs(got - fx * d / Z) <= 1e-9
    assert br.mssd(np.eye(3), [d, 0, Z], np.eye(3), [0, 0, Z], verts, [(np.eye(3), np.zeros(3))]) == pytest.approx(d, abs=1e-9)


def test_no_vertices_give_infinity():
    assert br.mssd(np.eye(3), [0, 0, 1], np.eye(3), [0, 0, 1], np.zeros((0, 3)), [(np.eye(3), np.zeros(3))]) == np.inf
    assert br.mspd(np.eye(3), [0, 0, 1], np.eye(3), [0, 0, 1], bc.CAM_K, np.zeros((0, 3)),
                   [(np.eye(3), np.zeros(3))]) == np.inf


# ------------------------------------------------------------------------------ VSD closed forms
def _blob():
    c = bc.vsd_case(33, 65, 1, 10, True, 2)
    return c["depth_gt"][0], c["K"][0], float(c["diameter"][0]), c["taus"]


def test_vsd_of_the_ground_truth_is_zero():
    gt, K, d, taus = _blob()
    counts, amb, _ = br.vsd_counts(gt, gt, gt, K, bc.DELTA, taus, d)
    mask = int((gt > 0).sum())
    assert mask > 100 and counts[0] == counts[1] == mask and not counts[2:].any() and amb == 0
    assert np.array_equal(br.vsd_errors(counts), np.zeros(10))


def test_vsd_of_an_empty_estimate_is_one():
    gt, K, d, taus = _blob()
    counts, _, _ = br.vsd_counts(np.zeros_like(gt), gt, gt, K, bc.DELTA, taus, d)
    assert counts[1] == 0 and counts[0] == int((gt > 0).sum())
    assert np.array_equal(br.vsd_errors(counts), np.ones(10))
    counts, _, _ = br.vsd_counts(np.full_like(gt, -1.0), gt, gt, K, bc.DELTA, taus, d)  # the renderer's empty
    assert counts[1] == 0 and np.array_equal(br.vsd_errors(counts), np.ones(10))


def test_vsd_behind_an_occluder_is_one():
    gt, K, d, taus = _blob()
    occluder = np.full_like(gt, 300.0)  # nearer than δ everywhere
    counts, _, _ = br.vsd_counts(gt, gt, occluder, K, bc.DELTA, taus, d)
    assert counts[0] == 0 and counts[1] == 0
    assert np.array_equal(br.vsd_errors(counts), np.ones(10))


def test_vsd_without_test_depth_sees_every_rendered_pixel():
    c = bc.vsd_case(33, 65, 1, 10, True, 2)
    gt, est = c["depth_gt"][0], c["depth_est"][0]
    counts, _, _ = br.vsd_counts(est, gt, np.zeros_like(gt), c["K"][0], bc.DELTA, c["taus"], float(c["diameter"][0]))
    assert counts[0] == int(((gt > 0) | (est > 0)).sum())
    assert counts[1] == int(((gt > 0) & (est > 0)).sum())


def test_vsd_cases_have_few_ambiguous_pixels():
    """The condition the GPU comparison leans on, for the committed seeds: ambiguous pixels ≤ 1 %
    of the union in every case (the GPU test allows a count to differ by their number)."""
    total_amb = total_union = 0
    for case in bc.vsd_case_list():
        counts, amb = bc.vsd_reference(*case)
        union = int(counts[:, 0].sum())
        print(case, "union", union, "ambiguous", amb)
        assert union > 0 and amb <= 0.01 * union, (case, amb, union)
        total_amb += amb
        total_union += union
    print("all cases: union", total_union, "ambiguous", total_amb)


# ------------------------------------------------------------------------------ recall
def _table():
    """Six GT instances, diameter 100: 0 exact, 1 small errors, 2 exactly on thresholds, 3 large,
    4 unmatched (+inf), 5 perfect but excluded by visib_fract."""
    vsd = np.array([[0.0] * 10, [0.07] * 10, [0.05] * 10, [0.9] * 10, [np.inf] * 10, [0.0] * 10])
    mssd = np.array([0.0, 7.0, 5.0, 90.0, np.inf, 0.0])   # thresholds 5, 10 … 50
    mspd = np.array([0.0, 12.0, 10.0, 900.0, np.inf, 0.0])  # thresholds 10, 20 … 100 at W = 1280
    targets = np.array([True, True, True, True, True, False])
    return vsd, mssd, mspd, np.full(6, 100.0), targets


def test_recall_on_a_hand_worked_table():
    vsd, mssd, mspd, diam, targets = _table()
    th = np.array(bm.BOP19_THETAS)
    # MSSD: θ·d = 5: only instance 0 (5.0 is ON the threshold: not correct, 7.0 above) → 1/5;
    # θ·d = 10 … 50: instances 0, 1, 2 → 3/5
    r = bm.recall(mssd, th[None] * diam[:, None], targets)
    assert np.array_equal(r, np.array([0.2] + [0.6] * 9))
    # the same table through plain thresholds, and the excluded instance changes nothing but n
    assert np.array_equal(bm.recall(mssd, th * 100.0, targets), r)
    assert np.array_equal(bm.recall(mssd, th * 100.0, np.ones(6, bool)), np.array([2 / 6] + [4 / 6] * 9))
    rv = bm.recall(vsd, th, targets)
    assert rv.shape == (10, 10) and np.array_equal(rv, np.tile(np.array([0.2, 0.6] + [0.6] * 8), (10, 1)))
    assert np.array_equal(bm.recall(mssd, th, np.zeros(6, bool)), np.zeros(10))


def test_average_recall_and_the_width_scaling():
    vsd, mssd, mspd, diam, targets = _table()
    ar = bm.average_recall(vsd, mssd, mspd, diam, 1280, targets)
    # MSPD at W = 1280: thresholds 10, 20 … 100: 10.0 on the first is not correct, 12.0 above it
    assert np.array_equal(ar["recall_mspd"], np.array([0.2] + [0.6] * 9))
    assert ar["AR_MSSD"] == pytest.approx(0.56) and ar["AR_MSPD"] == pytest.approx(0.56)
    assert ar["AR_VSD"] == pytest.approx(0.56)
    assert ar["AR"] == pytest.approx(0.56)
    # at W = 640 the thresholds are 5 … 50: 10.0 and 12.0 pass from the third / third on
    ar640 = bm.average_recall(vsd, mssd, mspd, diam, 640, targets)
    assert np.array_equal(ar640["recall_mspd"], np.array([0.2, 0.2] + [0.6] * 8))
    ref = br.average_recall(vsd, mssd, mspd, diam, 640, targets)
    for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR"):
        assert ar640[k] == pytest.approx(ref[k], abs=1e-15)
    assert np.array_equal(ar640["recall_vsd"], ref["recall_vsd"])


def test_end_to_end_perturbations_sit_away_from_the_thresholds():
    """The GPU end-to-end test compares recalls exactly, so no MSSD / MSPD error of its case may
    be within the fp32 tolerance of a threshold (its VSD margins are asserted there, on the
    renderer's own depth)."""
    c = bc.ar_case()
    mssd, mspd = bc.ar_reference()
    th = np.array(bm.BOP19_THETAS)
    big_t = float(np.abs(c["t_gt"]).max() + 150.0)
    tol_s = 32.0 * 2.0 ** -23 * (big_t + c["diameters"].max())
    tol_p = 64.0 * 2.0 ** -23 * 640.0
    ms = bc.threshold_margins(mssd, th[None] * c["diameters"][:, None])
    mp = bc.threshold_margins(mspd, np.array(bm.BOP19_MSPD_THETAS) * bc.AR_SIZE / 640.0)
    print("MSSD", mssd, "margin", ms, "tol", tol_s, "\nMSPD", mspd, "margin", mp, "tol", tol_p)
    assert ms > 10 * tol_s and mp > 10 * tol_p
    # the perturbations spread over the thresholds: some recall strictly between 0 and 1
    r = bm.recall(mssd, th[None] * c["diameters"][:, None], np.ones(8, bool))
    assert 0 < r[0] < r[-1] <= 1


@pytest.mark.parametrize("rows", [64, 48])
def test_end_to_end_vsd_errors_sit_away_from_the_thresholds(rows):
    """The same for VSD, on the CPU oracle's depth renders of the case (the GPU test repeats it
    on the HIP renderer's own): an ambiguous pixel moves an error by at most 2 / |U|; every error
    keeps that distance from every θ with one more ambiguous pixel than the case has."""
    from tests import render_cases as rc
    c = bc.ar_case()
    z = [np.stack([o["zbuf"] for o in rc.run_oracle(c["meshes"], c[r], c[t], c["K"], c["labels"], bc.AR_SIZE,
                                                    (True, True))]).astype(np.float32)
         for r, t in (("R_est", "t_est"), ("R_gt", "t_gt"))]
    counts, amb = bc.ar_vsd_reference(z[0], z[1], bc.ar_test_depth(z[1]), rows)
    margin = bc.vsd_threshold_margins(counts)
    print("union", counts[:, 0], "ambiguous", amb, "margins", margin)
    assert (counts[:, 0] > 200).all()
    assert (margin > 2.0 * (amb + 1) / counts[:, 0]).all()
    e = br.vsd_errors(counts)
    assert e.min() < 0.05 and e.max() == 1.0 and ((e > 0.1) & (e < 0.9)).sum() >= 20


# ------------------------------------------------------------------------------ files
def test_load_models_info_and_depth(tmp_path):
    from PIL import Image
    info = {"1": {"diameter": 172.0, "symmetries_discrete": [DISC_X]}, "13": {"diameter": 90.5}}
    p = tmp_path / "models_info.json"
    p.write_text(json.dumps(info))
    got = bop_eval.load_models_info(str(p))
    assert got == info and all(isinstance(k, str) for k in got)
    d = np.array([[0, 1, 65535], [7000, 8191, 12]], np.uint16)
    Image.fromarray(d).save(tmp_path / "000003.png")
    out = bop_eval.load_depth(str(tmp_path / "000003.png"), 0.1)
    assert out.dtype == np.float32 and out.shape == (2, 3)
    assert np.array_equal(out, d.astype(np.float32) * np.float32(0.1)) and out[0, 0] == 0
    assert np.array_equal(bop_eval.load_depth(str(tmp_path / "000003.png")), d.astype(np.float32))


# ------------------------------------------------------------------------------ evaluate_bop
class _Meshes:
    """What evaluate_bop reads of a Renderer."""
    def __init__(self, meshes):
        import torch
        self.meshes = {l: (torch.from_numpy(np.array(v)),) for l, v in meshes.items()}
        self.image_size = (16, 16)


def _restated_errors(batch, renderer):
    """The error functions by the restatement; the depth 'renders' are flat discs at t_z (the
    keys and the bookkeeping are under test here, not a rasteriser)."""
    n = len(batch["labels"])
    h, w = batch["depth_test"].shape[1:]
    yy, xx = np.mgrid[0:h, 0:w]
    v, s, p = [], [], []
    for i in range(n):
        lab = int(batch["labels"][i])
        verts = renderer.meshes[lab][0].numpy()
        syms = br.symmetry_set(batch["models_info"].get(str(lab + 1)))
        a = (batch["R_est"][i], batch["t_est"][i], batch["R_gt"][i], batch["t_gt"][i])
        s.append(br.mssd(*a, verts, syms))
        p.append(br.mspd(*a, batch["K"][i], verts, syms))
        disc = lambda t: np.where((xx - 8) ** 2 + (yy - 8) ** 2 <= 25, float(t[2]), 0.0)  # noqa: E731
        counts, _, _ = br.vsd_counts(disc(a[1]), disc(a[3]), batch["depth_test"][batch["frame_index"][i]],
                                     batch["K"][i], batch["delta"], batch["taus"], float(batch["diameters"][i]))
        v.append(br.vsd_errors(counts))
    return np.stack(v), np.array(s), np.array(p)


def test_evaluate_bop_keys_and_bookkeeping(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(5)
    meshes = {l: rng.uniform(-40, 40, (30, 3)).astype(np.float32) for l in range(3)}
    info = {"1": {"diameter": 100.0}, "2": {"diameter": 120.0, "symmetries_discrete": [DISC_X]},
            "3": {"diameter": 90.0}}
    K = [[300.0, 0, 8], [0, 300.0, 8], [0, 0, 1]]
    seq = "000048"
    scene_gt, scene_cam, scene_info, results = {}, {}, {}, []
    (tmp_path / seq / "depth").mkdir(parents=True)
    for img in (1, 2):
        objs, pl, pr, pt = [], [], [], []
        for k, oid in enumerate((1, 2, 3)):
            R, t = bc._random_rotation(rng), np.array([0.0, 0.0, 800.0 + 10 * k])
            objs.append(dict(obj_id=oid, cam_R_m2c=R.reshape(-1).tolist(), cam_t_m2c=t.tolist()))
            if img == 2 and oid == 3:
                continue  # image 2 misses object 3
            pl.append(oid - 1)
            pr.append(R)
            pt.append(t + (0.5 if oid == 1 else 30.0))
        scene_gt[str(img)], scene_cam[str(img)] = objs, dict(cam_K=np.array(K).reshape(-1).tolist(), depth_scale=0.5)
        scene_info[str(img)] = [dict(visib_fract=0.9), dict(visib_fract=0.05 if img == 1 else 0.8),
                                dict(visib_fract=0.5)]
        Image.fromarray(np.full((16, 16), 1600 + 20 * img, np.uint16)).save(tmp_path / seq / "depth" / f"{img:06d}.png")
        results.append(dict(img_metas=dict(img_path=f"{tmp_path}/{seq}/rgb/{img:06d}.png"),
                            pred=dict(labels=np.array(pl), rotations=np.array(pr, np.float32),
                                      translations=np.array(pt, np.float32))))
    gt = {seq: dict(pose=scene_gt, camera=scene_cam, gt_info=scene_info)}
    names = ["a", "b", "c"]
    out = bop_eval.evaluate_bop(results, gt, info, _Meshes(meshes), str(tmp_path), class_names=names,
                                error_fn=_restated_errors)
    keys = {f"{n}/{m}" for n in ["all"] + names for m in ("AR", "AR_VSD", "AR_MSSD", "AR_MSPD")}
    keys |= {f"all/mssd_{k:02d}" for k in range(5, 55, 5)} | {f"all/mspd_{k:02d}" for k in range(5, 55, 5)}
    assert set(out) == keys
    assert all(isinstance(v, float) for v in out.values())
    # five targets (one of six GTs is below visib_fract 0.1); class c has one of two estimated
    assert out["all/AR"] == pytest.approx((out["all/AR_VSD"] + out["all/AR_MSSD"] + out["all/AR_MSPD"]) / 3)
    # class a: 0.5 mm off in x, y, z: MSSD 0.87 mm < 5 mm: correct at every threshold
    assert out["a/AR_MSSD"] == 1.0
    # class c: the unmatched GT of image 2 is a target that is never correct: recall ≤ 1/2
    assert 0.0 <= out["c/AR_MSSD"] <= 0.5 and 0.0 <= out["c/AR_VSD"] <= 0.5
    # a loader in place of the root gives the same numbers (depth_scale 0.5 applied by the root reader)
    loader = lambda s, i: np.full((16, 16), (1600 + 20 * i) * 0.5, np.float32)  # noqa: E731
    assert bop_eval.evaluate_bop(results, gt, info, _Meshes(meshes), loader, class_names=names,
                                 error_fn=_restated_errors) == out
    # without scene_gt_info every GT is a target
    gt2 = {seq: dict(pose=scene_gt, camera=scene_cam)}
    out2 = bop_eval.evaluate_bop(results, gt2, info, _Meshes(meshes), loader, error_fn=_restated_errors)
    assert set(out2) == {k for k in keys if k.startswith("all/")}
    # a (0.87 mm) and b (52 mm < 60) in both images; c is 52 mm > 45 in one and missing in the other
    assert out2["all/mssd_50"] == pytest.approx(4 / 6)
